"""Host-side mirrors of the reference's multi-view voxel lifting:

* ``point_sample``  -- mmdet3d/models/fusion_layers/point_fusion.py:14-106
* ``mv_feature_transformation`` -- the sampling/reduction part of
  ``MultiViewDfM.feature_transformation`` (mmdet3d/models/detectors/
  multiview_dfm.py:119-208, ``valid_sample=True``)
* ``voxel_centers`` -- the sample points the detector takes from
  ``AlignedAnchor3DRangeGenerator`` (core/anchor/anchor_3d_generator.py:285-332)

One HIP launch (``dfm_point_sample_mv_fwd``) replaces the per-(frame, view)
``point_sample`` calls, the stack/sum/count/divide passes and the permute.
"""
import ctypes

import numpy as np
import torch

from . import _capi
from ._launch import DTYPES, STREAM, WS, launch, require_gpu, try_launch, upload


def voxel_centers(voxel_range, n_voxels):
    """(Nz*Ny*Nx, 3) fp32 voxel centres, ordered z-major then y then x, computed
    with the torch ops of AlignedAnchor3DRangeGenerator.anchors_single_range
    (align_corner=False) on the CPU."""
    nx, ny, nz = (int(v) for v in n_voxels)
    rng = torch.tensor(voxel_range, dtype=torch.float32)
    z = torch.linspace(rng[2], rng[5], nz + 1)
    y = torch.linspace(rng[1], rng[4], ny + 1)
    x = torch.linspace(rng[0], rng[3], nx + 1)
    z = z + (z[1] - z[0]) / 2
    y = y + (y[1] - y[0]) / 2
    x = x + (x[1] - x[0]) / 2
    zz, yy, xx = torch.meshgrid(z[:nz], y[:ny], x[:nx], indexing='ij')
    return torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3).contiguous()


_CENTERS = {}


def _device_voxel_centers(voxel_range, n_voxels, device):
    """voxel centres on the device, built and uploaded once per (range, grid, device): the
    reference regenerates the anchor grid every forward (multiview_dfm.py:122-123); 9.5 MB per
    call through a blocking H2D copy is a pipeline stall"""
    key = (tuple(float(v) for v in voxel_range), tuple(int(v) for v in n_voxels), str(device))
    pts = _CENTERS.get(key)
    if pts is None:
        if len(_CENTERS) > 16:
            _CENTERS.clear()
        pts = _CENTERS[key] = voxel_centers(voxel_range, n_voxels).to(device)
    return pts


def _scale_xy(img_scale_factor):
    if torch.is_tensor(img_scale_factor) or isinstance(img_scale_factor, np.ndarray):
        s = np.asarray(torch.as_tensor(img_scale_factor).detach().cpu(), dtype=np.float32).reshape(-1)
        return (float(s[0]), float(s[1])) if s.size >= 2 else (float(s[0]), float(s[0]))
    return float(img_scale_factor), float(img_scale_factor)


def _crop_xy(img_crop_offset):
    if torch.is_tensor(img_crop_offset) or isinstance(img_crop_offset, (np.ndarray, list, tuple)):
        c = np.asarray(torch.as_tensor(img_crop_offset).detach().cpu(), dtype=np.float32).reshape(-1)
        return float(c[0]), float(c[1])
    return float(img_crop_offset), float(img_crop_offset)


def _views_channels_last(x):
    """(B, F*Nv, C, H, W) whose every view is stored (H, W, C) -- what ``.view(B, F*Nv, C, H, W)`` of
    a channels_last image backbone / neck output is -- with whole 16-byte channel blocks"""
    if x.dim() != 5 or x.is_contiguous():
        return False
    B, V, C, H, W = x.shape
    return (x.stride() == (V * H * W * C, H * W * C, 1, W * C, C) and C % (16 // x.element_size()) == 0 and
            x.data_ptr() % 16 == 0)


def _make_desc(feats, npoints, nxyz, num_views, num_frames, scale, crop, flip, pad_shape, aligned,
               aggregate, valid_sample):
    nvf, C, Hf, Wf = feats.shape[-4:]
    assert nvf == num_views * num_frames
    desc = _capi.MvDesc()
    desc.num_views, desc.num_frames, desc.channels = num_views, num_frames, C
    desc.feat_h, desc.feat_w = Hf, Wf
    desc.nx, desc.ny, desc.nz = nxyz if nxyz is not None else (0, 0, 0)
    desc.num_points = npoints
    desc.scale_x, desc.scale_y = scale
    desc.crop_x, desc.crop_y = crop
    desc.flip = 1 if flip else 0
    desc.pad_h, desc.pad_w = float(pad_shape[0]), float(pad_shape[1])
    desc.mode = 1 if aligned else 0
    desc.aggregate = 1 if aggregate == 'concat' else 0
    desc.valid_sample = 1 if valid_sample else 0
    desc.dtype = DTYPES[feats.dtype]
    return desc


def _reverse_3d_flow(points, coord_type, img_meta):
    """``apply_3d_transformation(points, coord_type, img_meta, reverse=True)``
    (fusion_layers/coord_transform.py:9-95) on the device, operation by operation in the
    reference's order: the recorded ``transformation_3d_flow`` undone back to front -- 'T' adds
    -pcd_trans, 'S' multiplies by 1/pcd_scale_factor, 'R' multiplies by inverse(pcd_rotation) from
    the right (as an explicit fp32 multiply-add chain over x, y, z, not a BLAS call), 'HF' / 'VF'
    negate the BEV axes of the coordinate type (core/points/{lidar,cam,depth}_points.py flip).
    Returns ``points`` itself when there is nothing to undo."""
    flow = (img_meta or {}).get('transformation_3d_flow') or []
    if not flow:
        return points
    axes = {'LIDAR': (1, 0), 'CAMERA': (0, 2), 'DEPTH': (0, 1)}[coord_type]  # (horizontal, vertical)
    p = points.clone()
    for op in flow[::-1]:
        if op == 'T':
            t = torch.as_tensor(img_meta.get('pcd_trans', [0.0, 0.0, 0.0]), dtype=torch.float32)
            p[:, :3] += (-t).to(p.device)
        elif op == 'S':
            p[:, :3] *= 1.0 / img_meta.get('pcd_scale_factor', 1.0)
        elif op == 'R':
            r = torch.as_tensor(img_meta['pcd_rotation'], dtype=torch.float32) if 'pcd_rotation' in img_meta \
                else torch.eye(3)
            ri = torch.inverse(r).to(p.device)
            x, y, z = p[:, 0].clone(), p[:, 1].clone(), p[:, 2].clone()
            for j in range(3):
                p[:, j] = torch.addcmul(torch.addcmul(x * ri[0, j], y, ri[1, j]), z, ri[2, j])
        elif op == 'HF':
            if img_meta.get('pcd_horizontal_flip', False):
                p[:, axes[0]] = -p[:, axes[0]]
        elif op == 'VF':
            if img_meta.get('pcd_vertical_flip', False):
                p[:, axes[1]] = -p[:, axes[1]]
        else:
            raise KeyError(f'unknown transformation_3d_flow entry {op!r}')
    return p


class _MvFn(torch.autograd.Function):
    """feats (B, F*Nv, C, Hf, Wf); one launch per sample (its own image transform in
    ``descs[b]``) straight into one (B, ...) output; proj (B, F*Nv, 16), ori_w (B, F*Nv);
    points (N, 3) shared by the batch or (B, N, 3) per sample (3-D augmentation flows)."""

    @staticmethod
    def forward(ctx, feats, points, proj, ori_w, descs, nxyz, want_valid, channels_last=False):
        lib = _capi.lib()
        device = feats.device
        B = feats.shape[0]
        d0 = descs[0]
        c_out = d0.channels * (d0.num_frames if d0.aggregate else 1)
        if nxyz is not None and channels_last:
            # (B, Nx, Ny, Nz, C) in memory = (B, C, Nx, Ny, Nz) channels_last_3d
            out = torch.empty((B,) + tuple(nxyz) + (c_out,), dtype=feats.dtype, device=device).permute(0, 4, 1, 2, 3)
            for d in descs:
                d.out_channels_last = 1
        elif nxyz is not None:
            out = torch.empty((B, c_out) + tuple(nxyz), dtype=feats.dtype, device=device)
        else:
            out = torch.empty((B, points.shape[-2], c_out), dtype=feats.dtype, device=device)
        valid = torch.empty((B, points.shape[-2]), dtype=torch.uint8, device=device) if want_valid else None
        nbytes = lib.dfm_point_sample_mv_workspace_bytes(ctypes.byref(d0))
        # the whole batch in one launch when the lanes-per-voxel kernel covers the call (channels-last
        # views and volume, nearest sampling); DFM_ERR_UNSUPPORTED: one launch per sample below
        batched = d0.feats_channels_last and d0.mode == 0 and d0.valid_sample and \
            (nxyz is None or channels_last) and proj.is_contiguous() and ori_w.is_contiguous() and \
            try_launch('dfm_point_sample_mv_fwd_batched', (_capi.MvDesc * B)(*descs), B, feats, points,
                       1 if points.dim() == 3 else 0, proj, ori_w, out, valid, STREAM)
        for b in range(0 if batched else B):
            launch('dfm_point_sample_mv_fwd', descs[b], feats[b], points[b] if points.dim() == 3 else points,
                   proj[b], ori_w[b], out[b], valid[b] if want_valid else None, WS, STREAM, ws_bytes=nbytes)
        ctx.descs = descs  # (the backward reads a (C, N) gradient: grad_out.contiguous() below)
        ctx.meta = (feats.shape, feats.dtype)
        ctx.save_for_backward(points, proj, ori_w)
        if want_valid:
            ctx.mark_non_differentiable(valid)
        return out, valid

    @staticmethod
    def backward(ctx, grad_out, _grad_valid):
        points, proj, ori_w = ctx.saved_tensors
        lib = _capi.lib()
        shape, dtype = ctx.meta
        device = grad_out.device
        go = grad_out.contiguous().to(dtype)
        gf = torch.zeros(shape, dtype=torch.float32, device=device)
        nbytes = lib.dfm_point_sample_mv_bwd_workspace_bytes(ctypes.byref(ctx.descs[0]))
        for b in range(shape[0]):
            launch('dfm_point_sample_mv_bwd', ctx.descs[b], go[b], points[b] if points.dim() == 3 else points,
                   proj[b], ori_w[b], gf[b], WS, STREAM, ws_bytes=nbytes)
        return gf.to(dtype), None, None, None, None, None, None, None


def point_sample(img_meta,
                 img_features,
                 points,
                 proj_mat,
                 coord_type,
                 img_scale_factor,
                 img_crop_offset,
                 img_flip,
                 img_pad_shape,
                 img_shape,
                 aligned=True,
                 padding_mode='zeros',
                 align_corners=True,
                 valid_flag=False):
    """Drop-in for the reference ``point_sample``: (N, C) features of one view
    [+ (N,) bool validity when ``valid_flag``]."""
    if padding_mode != 'zeros' or not align_corners:
        raise NotImplementedError('only padding_mode="zeros", align_corners=True (what DfM uses)')
    require_gpu(img_features, 'img_features')
    assert img_features.dim() == 4 and img_features.shape[0] == 1
    device = img_features.device
    feats = img_features.contiguous()
    pts = torch.as_tensor(points, dtype=torch.float32).to(device).contiguous()
    pts = _reverse_3d_flow(pts, coord_type, img_meta).contiguous()  # point_fusion.py:57-58
    proj = torch.as_tensor(proj_mat, dtype=torch.float32).reshape(1, 16).to(device).contiguous()
    ori_w = torch.tensor([float(img_shape[1])], dtype=torch.float32, device=device)
    desc = _make_desc(feats, pts.shape[0], None, 1, 1, _scale_xy(img_scale_factor),
                      _crop_xy(img_crop_offset), img_flip, img_pad_shape, aligned, 'mean', valid_flag)
    out, valid = _MvFn.apply(feats[None], pts, proj[None], ori_w[None], [desc], None, valid_flag)
    if valid_flag:
        return out[0], valid[0].bool()
    return out[0]


def mv_feature_transformation(batch_feats, img_metas, num_views, num_frames, voxel_range, n_voxels,
                              temporal_aggregate='mean', points=None, valid_sample=True,
                              memory_format=torch.contiguous_format):
    """(B, F*Nv, C, Hf, Wf) view features -> (B, C or C*F, Nx, Ny, Nz) voxel volume,
    the tensor the reference hands to ``neck_3d`` (multiview_dfm.py:206-209).
    ``memory_format=torch.channels_last_3d`` (extension): the same tensor stored (B, Nx, Ny, Nz, C),
    what the NDHWC / MFMA neck convolutions read -- written directly, no conversion copy."""
    require_gpu(batch_feats, 'batch_feats')
    device = batch_feats.device
    if points is None:
        points = _device_voxel_centers(voxel_range, n_voxels, device)
    points = torch.as_tensor(points, dtype=torch.float32).to(device).contiguous()
    nxyz = tuple(int(v) for v in n_voxels)
    nvf = num_views * num_frames
    # channels_last view features are sampled in place (they are the kernel's pixel-major layout)
    feats_cl = _views_channels_last(batch_feats)
    feats = batch_feats if feats_cl else batch_feats.contiguous()
    descs, proj, ori_w = [], [], []
    for img_meta in img_metas:
        if 'scale_factor' in img_meta:
            sf = img_meta['scale_factor']
            scale = _scale_xy(sf[:2] if isinstance(sf, np.ndarray) and len(sf) >= 2 else sf)
        else:
            scale = (1.0, 1.0)
        flip = img_meta.get('flip', False)
        crop = _crop_xy(img_meta['img_crop_offset']) if 'img_crop_offset' in img_meta else (0.0, 0.0)
        l2i = img_meta['ori_lidar2img']
        if torch.is_tensor(l2i):   # staged by data_geometry.stage_geometry: read where it lies
            proj.append(l2i[:nvf].to(torch.float32).reshape(nvf, 16))
        else:
            proj.append(np.asarray(l2i[:nvf], dtype=np.float32).reshape(nvf, 16))
        ori_w.append([float(img_meta['img_shape'][i][1]) for i in range(nvf)])
        descs.append(_make_desc(feats, points.shape[0], nxyz, num_views, num_frames, scale, crop,
                                flip, img_meta['input_shape'], False, temporal_aggregate,
                                valid_sample))
        descs[-1].feats_channels_last = 1 if feats_cl else 0
    # one upload for the whole batch's matrices
    if all(torch.is_tensor(p_) for p_ in proj):
        proj = torch.stack([p_.to(device) for p_ in proj]).contiguous()   # device tensors: no host round trip
    else:
        proj = upload(torch.from_numpy(np.stack([p_.detach().cpu().numpy() if torch.is_tensor(p_) else p_
                                                  for p_ in proj])), device)
    ori_w = upload(torch.tensor(ori_w, dtype=torch.float32), device)
    if any(m.get('transformation_3d_flow') for m in img_metas):
        # point_sample undoes each sample's own 3-D augmentation first (point_fusion.py:57-58)
        points = torch.stack([_reverse_3d_flow(points, 'LIDAR', m) for m in img_metas]).contiguous()
    out, _ = _MvFn.apply(feats, points, proj, ori_w, descs, nxyz, False,
                         memory_format == torch.channels_last_3d)
    return out


def voxel_sample(voxel_features,
                 voxel_range,
                 voxel_size,
                 depth_samples,
                 proj_mat,
                 downsample_factor,
                 img_scale_factor,
                 img_crop_offset,
                 img_flip,
                 img_pad_shape,
                 img_shape,
                 aligned=True,
                 padding_mode='zeros',
                 align_corners=True,
                 proj_inv=None):
    """Drop-in for the reference ``voxel_sample`` (point_fusion.py:324-410):
    (1, C, Nx, Ny, Nz) voxel features -> (1, C, D, H_out, W_out) frustum features.

    ``proj_inv`` (extension): a precomputed fp32 inverse of ``proj_mat``.  By default
    it is taken with torch.inverse on the host like the reference does
    (utils.py:241); for a general 4x4 LAPACK's result can differ in the last bits
    between CPU models, so bit-exact replays of a fixture pass the stored inverse."""
    if padding_mode != 'zeros' or not align_corners:
        raise NotImplementedError('only padding_mode="zeros", align_corners=True')
    require_gpu(voxel_features, 'voxel_features')
    assert voxel_features.dim() == 5 and voxel_features.shape[0] == 1
    device = voxel_features.device
    vox = voxel_features.contiguous()
    depths = torch.as_tensor(depth_samples, dtype=torch.float32)[::downsample_factor]
    depths = depths.to(device).contiguous()
    desc = _capi.VsDesc()
    desc.channels, desc.nx, desc.ny, desc.nz = vox.shape[1:]
    desc.num_depths = depths.numel()
    desc.h_out = round(img_pad_shape[0] / downsample_factor)
    desc.w_out = round(img_pad_shape[1] / downsample_factor)
    desc.downsample_factor = float(downsample_factor)
    desc.scale_x, desc.scale_y = _scale_xy(img_scale_factor)
    desc.crop_x, desc.crop_y = _crop_xy(img_crop_offset)
    desc.flip, desc.ori_w = (1 if img_flip else 0), float(img_shape[1])
    for i, v in enumerate(np.asarray(voxel_range, dtype=np.float32).reshape(6)):
        desc.voxel_range[i] = float(v)
    for i, v in enumerate(np.asarray(voxel_size, dtype=np.float32).reshape(3)):
        desc.voxel_size[i] = float(v)
    inv = torch.as_tensor(proj_inv, dtype=torch.float32) if proj_inv is not None else \
        torch.inverse(torch.as_tensor(proj_mat, dtype=torch.float32).detach().cpu())  # utils.py:241
    for i, v in enumerate(inv.reshape(16).tolist()):
        desc.proj_inv[i] = v
    desc.mode = 1 if aligned else 0
    desc.dtype = DTYPES[vox.dtype]
    return _VoxelSampleFn.apply(vox, depths, desc)


class _VoxelSampleFn(torch.autograd.Function):
    """dfm_voxel_sample_fwd / _bwd (gradient w.r.t. the voxel features)"""

    @staticmethod
    def forward(ctx, vox, depths, desc):
        device = vox.device
        out = torch.empty((1, desc.channels, desc.num_depths, desc.h_out, desc.w_out), dtype=vox.dtype,
                          device=device)
        launch('dfm_voxel_sample_fwd', desc, vox, depths, out, STREAM)
        ctx.desc, ctx.meta = desc, (vox.shape, vox.dtype)
        ctx.save_for_backward(depths)
        return out

    @staticmethod
    def backward(ctx, gout):
        (depths,) = ctx.saved_tensors
        shape, dtype = ctx.meta
        device = gout.device
        go = gout.contiguous().to(dtype)
        gv = torch.zeros(shape, dtype=torch.float32, device=device)
        launch('dfm_voxel_sample_bwd', ctx.desc, go, depths, gv, STREAM)
        return gv.to(dtype), None, None


def _pair_rows(inv, scales, crops, flips, img_shapes, num_views):
    """the (B * Nv, VS_PAIR_FLOATS) rows of dfm_voxel_sample_mv_*: ``inv`` (B * Nv, 16) or None (filled on the
    device), then scale, crop, ori_w and flip of each pair"""
    B = len(scales)
    rows = np.zeros((B * num_views, _capi.VS_PAIR_FLOATS), dtype=np.float32)
    if inv is not None:
        rows[:, :16] = inv
    for b in range(B):
        for v in range(num_views):
            rows[b * num_views + v, 16:22] = (*scales[b], *crops[b], float(img_shapes[b][v][1]),
                                              1.0 if flips[b] else 0.0)
    return rows


def voxel_sample_mv(volume,
                    voxel_range,
                    voxel_size,
                    depth_samples,
                    proj_mats,
                    downsample_factor,
                    img_scale_factors,
                    img_crop_offsets,
                    img_flips,
                    img_pad_shape,
                    img_shapes,
                    num_views,
                    memory_format=torch.contiguous_format,
                    proj_invs=None):
    """``voxel_sample`` (aligned=True) for every (sample, view) pair of a batch in one launch: the loop of
    ``MultiViewDfM.feature_transformation`` with its two ``torch.cat`` (multiview_dfm.py:220-256).

    ``volume`` (B, C, Nx, Ny, Nz) fp32 / bf16, contiguous or channels_last_3d (read where it lies) ->
    (B * Nv, C, D, h_out, w_out), pair b * Nv + v from sample b and view v; bit for bit what B * Nv calls of
    ``voxel_sample`` on ``volume[b][None]`` give, concatenated.  Differentiable with respect to ``volume`` (the
    views of a sample are summed with fp32 atomics: the last bits of the gradient are not fixed from run to run).

    ``proj_mats``: the ORIGINAL lidar2img matrices, ``proj_mats[b][v]`` a 4x4 (nested lists, arrays, one
    (B, Nv, 4, 4) tensor, or per-sample tensors).  Host matrices are inverted one by one with ``torch.inverse``
    in fp32 on the host -- the reference's op (utils.py:241), the bits the single call uses -- and uploaded
    together, once.  Matrices that live on the device (``data_geometry.stage_geometry``) stay there: they are
    inverted by ``dfm_camera_prepare``, which agrees with the host inverse to fp32 rounding, not bit for bit.
    ``proj_invs`` (B, Nv, 4, 4): precomputed fp32 inverses (bit-exact replays of a fixture).
    ``img_scale_factors`` / ``img_crop_offsets`` / ``img_flips``: one entry per sample, as ``voxel_sample`` takes
    them; ``img_pad_shape``: (h, w) shared by the batch (a list with one equal entry per sample is accepted);
    ``img_shapes[b][v]``: (h, w, ...) of the view before padding.
    ``memory_format=torch.channels_last_3d``: the result stored (B * Nv, D, h_out, w_out, C), what
    ``MfmaConv3dTo1`` reads."""
    require_gpu(volume, 'volume')
    assert volume.dim() == 5
    if volume.dtype not in DTYPES:
        raise TypeError(f'volume must be float32 or bfloat16, got {volume.dtype}')
    device = volume.device
    B, C = volume.shape[:2]
    num_views = int(num_views)
    P = B * num_views
    if not (len(img_scale_factors) == len(img_crop_offsets) == len(img_flips) == len(img_shapes) == B):
        raise ValueError('one scale factor, crop offset, flip and img_shapes entry per sample of the volume')
    pads = list(img_pad_shape) if isinstance(img_pad_shape[0], (tuple, list, torch.Size, np.ndarray)) else [img_pad_shape]
    pads = {(int(p_[0]), int(p_[1])) for p_ in pads}
    if len(pads) != 1:
        raise ValueError(f'the samples of a batch share one padded shape, got {sorted(pads)}')
    pad = pads.pop()
    if volume.is_contiguous():
        vox, vcl = volume, 0
    elif volume.is_contiguous(memory_format=torch.channels_last_3d):
        vox, vcl = volume, 1
    else:
        vox, vcl = volume.contiguous(), 0
    downsample_factor = int(downsample_factor)
    depths = upload(torch.as_tensor(depth_samples, dtype=torch.float32).detach()[::downsample_factor], device)
    depths = depths.contiguous()
    scales = [_scale_xy(s) for s in img_scale_factors]
    crops = [_crop_xy(c) for c in img_crop_offsets]
    on_device = proj_invs is None and (
        (torch.is_tensor(proj_mats) and proj_mats.is_cuda) or
        (not torch.is_tensor(proj_mats) and all(torch.is_tensor(m) and m.is_cuda for m in proj_mats)))
    if on_device:
        mats = proj_mats if torch.is_tensor(proj_mats) else torch.stack([m[:num_views] for m in proj_mats])
        mats = mats[:, :num_views].to(device=device, dtype=torch.float32).reshape(P, 4, 4).contiguous()
        pad4, inv = torch.empty((P, 16), dtype=torch.float32, device=device), \
            torch.empty((P, 16), dtype=torch.float32, device=device)
        launch('dfm_camera_prepare', mats, 4, 4, P, pad4, inv, STREAM)
        pairs = upload(torch.from_numpy(_pair_rows(None, scales, crops, img_flips, img_shapes, num_views)), device)
        pairs[:, :16] = inv
    else:
        def host(m):
            return torch.as_tensor(np.asarray(m.detach().cpu() if torch.is_tensor(m) else m, dtype=np.float32))
        if proj_invs is not None:
            inv = torch.stack([host(proj_invs[b][v]) for b in range(B) for v in range(num_views)])
        else:
            inv = torch.stack([torch.inverse(host(proj_mats[b][v]))   # utils.py:241, one matrix at a time
                               for b in range(B) for v in range(num_views)])
        pairs = upload(torch.from_numpy(_pair_rows(inv.reshape(P, 16).numpy(), scales, crops, img_flips,
                                                    img_shapes, num_views)), device)
    desc = _capi.VsMvDesc()
    desc.batch, desc.num_views, desc.channels = B, num_views, C
    desc.nx, desc.ny, desc.nz = vox.shape[2:]
    desc.num_depths = depths.numel()
    desc.h_out, desc.w_out = round(pad[0] / downsample_factor), round(pad[1] / downsample_factor)
    desc.downsample_factor = float(downsample_factor)
    for i, v in enumerate(np.asarray(voxel_range, dtype=np.float32).reshape(6)):
        desc.voxel_range[i] = float(v)
    for i, v in enumerate(np.asarray(voxel_size, dtype=np.float32).reshape(3)):
        desc.voxel_size[i] = float(v)
    desc.dtype = DTYPES[vox.dtype]
    desc.volume_channels_last = vcl
    desc.out_channels_last = 1 if memory_format == torch.channels_last_3d else 0
    return _VoxelSampleMvFn.apply(vox, depths, pairs, desc)


class _VoxelSampleMvFn(torch.autograd.Function):
    """dfm_voxel_sample_mv_fwd / _bwd (gradient w.r.t. the volume, in the volume's layout)"""

    @staticmethod
    def forward(ctx, vox, depths, pairs, desc):
        device = vox.device
        P, C = desc.batch * desc.num_views, desc.channels
        lattice = (desc.num_depths, desc.h_out, desc.w_out)
        if desc.out_channels_last:
            out = torch.empty((P,) + lattice + (C,), dtype=vox.dtype, device=device).permute(0, 4, 1, 2, 3)
        else:
            out = torch.empty((P, C) + lattice, dtype=vox.dtype, device=device)
        launch('dfm_voxel_sample_mv_fwd', desc, pairs, vox, depths, out, STREAM)
        ctx.desc, ctx.meta = desc, (vox.shape, vox.dtype)
        ctx.save_for_backward(depths, pairs)
        return out

    @staticmethod
    def backward(ctx, gout):
        depths, pairs = ctx.saved_tensors
        (B, C, nx, ny, nz), dtype = ctx.meta
        desc = ctx.desc
        device = gout.device
        go = gout.to(dtype)
        if desc.out_channels_last:
            go = go.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
        else:
            go = go.contiguous()
        if desc.volume_channels_last:
            gv = torch.zeros((B, nx, ny, nz, C), dtype=torch.float32, device=device).permute(0, 4, 1, 2, 3)
        else:
            gv = torch.zeros((B, C, nx, ny, nz), dtype=torch.float32, device=device)
        launch('dfm_voxel_sample_mv_bwd', desc, pairs, go, depths, gv, STREAM)
        return gv.to(dtype), None, None, None
