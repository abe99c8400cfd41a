/* dfm_hip_optim.h -- the part of the C ABI of libdfm_hip.so that ends a training iteration: the global L2 norm of the
 * gradients, the clip against it and the AdamW update, over ALL parameters in one launch each (mmcv's OptimizerHook:
 * torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2), then torch.optim.AdamW.step()).
 * Included by dfm_hip.h (inside its extern "C" block, after DFM_API and the status codes): include that header, not
 * this one.  Bound by depth-from-motion_amd/_capi.py under this header's name. */
#ifndef DFM_HIP_OPTIM_H
#define DFM_HIP_OPTIM_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

#define DFM_OPTIM_THREADS 256 /* lanes of a workgroup */
#define DFM_OPTIM_CHUNK 8192  /* elements of one tensor that one workgroup owns: 32 per lane */
#define DFM_OPTIM_ZERO_GRADS 1 /* flags of dfm_adamw_step: store zeros over the gradients just read */

/* One row of the MULTI-TENSOR TABLE, which lives in DEVICE memory: one parameter tensor of the step.  The five arrays
 * are DEVICE ADDRESSES kept as int64_t (the table is plain data that the host fills and copies over); each holds
 * numel elements in the same (storage) order.  param and grad have the type dtype (DFM_F32 or DFM_BF16); exp_avg,
 * exp_avg_sq and master are always FP32.  master is 0 for an FP32 parameter (the parameter is its own master); a BF16
 * parameter with master 0 is widened, updated and rounded back, which is torch's own BF16 step and loses every update
 * below half a BF16 ulp.  dfm_grad_sqnorm and dfm_grad_scale read only grad, numel and dtype.
 * Alignment: param and grad need the alignment of their type only (4 / 2 bytes) -- a parameter that is a view at an
 * odd element offset of its storage is served; the FP32 arrays need 4 bytes.  An array that is 16-byte aligned is read
 * and written in 16-byte vectors, any other one element by element; that is decided per array, since the five arrays
 * of one tensor need not share a misalignment (the gradient of an offset view is a fresh allocation), and the
 * last numel % 4 (FP32) or numel % 8 (BF16) elements of a tensor are a scalar tail.
 * The scalars are torch's, computed on the host in double and rounded ONCE to FP32 (torch/optim/adam.py
 * _single_tensor_adam; t is this tensor's step count AFTER the increment):
 *   decay = 1 - lr * weight_decay;  step_size = lr / (1 - beta1^t);  bc2_sqrt = sqrt(1 - beta2^t);
 *   lerp_weight = 1 - beta1;  beta2;  one_minus_beta2 = 1 - beta2;  eps.
 * They are per tensor because lr, the decay and t are: mmcv's paramwise_cfg makes one parameter group per parameter,
 * and a parameter without a gradient does not advance its t. */
typedef struct dfm_optim_tensor {
    int64_t param, grad, exp_avg, exp_avg_sq, master;
    int64_t numel;
    int32_t dtype, reserved;
    float decay, step_size, bc2_sqrt, lerp_weight, beta2, one_minus_beta2, eps, reserved_f;
} dfm_optim_tensor;

/* The CHUNK TABLE, in device memory too: num_chunks pairs of int32 (tensor, chunk).  Workgroup w of every kernel here
 * owns the elements [chunk * DFM_OPTIM_CHUNK, min(numel, (chunk + 1) * DFM_OPTIM_CHUNK)) of table[tensor], so the grid
 * is the number of chunks whatever the number of tensors.  A pair that names no tensor of the table, or a chunk past
 * its tensor's end, makes its workgroup do nothing.  THE CALLER guarantees that the addresses of the table hold numel
 * elements: nothing here can check device memory from the host. */

/* partials[w] = the sum of the squares of workgroup w's gradient elements, accumulated in FP32: each lane adds its
 * elements in index order (at most DFM_OPTIM_CHUNK / DFM_OPTIM_THREADS + 1 of them), the 64 lanes of a wave are added
 * by a 6-level butterfly, the 4 waves in order through LDS.  No atomics: the same gradients give the same bits.
 * One launch.  partials: num_chunks floats. */
DFM_API int dfm_grad_sqnorm(const void *table, int32_t num_tensors, const void *chunks, int64_t num_chunks,
                            float *partials, void *stream);

/* The AdamW update of every tensor of the table, one launch.
 * With partials (and then norm_out) given, every workgroup first adds the partials in one fixed order -- lane l adds
 * partials[l], [l + 256], ... in order, then the butterfly and the 4 waves as above -- so all of them hold the same
 * bits: norm = sqrtf(sum);  coef = (1 / (norm + 1e-6f)) * max_norm -- the two roundings of torch's scalar / tensor,
 * which is reciprocal() * scalar -- replaced by 1 where it is greater than 1 (a NaN stays, as torch.clamp keeps it; an
 * infinite norm gives 0).  Workgroup 0 stores norm to norm_out[0].  With partials NULL
 * there is no clipping: coef = 1 and norm_out is not touched.
 * Then per element, in FP32 with one rounding per operation (no contraction), g = grad * coef:
 *   p32 = p32 * decay
 *   m   = lerp_weight < 0.5 ? m + lerp_weight * (g - m) : g - (g - m) * (1 - lerp_weight)        (torch's lerp)
 *   v   = v * beta2 + (one_minus_beta2 * g) * g
 *   p32 = p32 + ((-step_size) * m) / (sqrtf(v) / bc2_sqrt + eps)
 * p32 is param itself for DFM_F32; for DFM_BF16 it is master (else the widened param), and param receives bf16(p32),
 * round to nearest even.
 * grad is read once and, with DFM_OPTIM_ZERO_GRADS in flags, overwritten with zeros; without it grad is not written
 * (it stays unscaled).  Non-finite values take their IEEE course, as in torch.
 * num_chunks == 0 returns DFM_OK and launches nothing (norm_out is then not written). */
DFM_API int dfm_adamw_step(const void *table, int32_t num_tensors, const void *chunks, int64_t num_chunks,
                           const float *partials, float max_norm, float *norm_out, int32_t flags, void *stream);

/* grad = grad * coef in place (rounded to grad's type), coef and norm_out from the partials exactly as above: the
 * second launch of a stand-alone clip_grad_norm_. */
DFM_API int dfm_grad_scale(const void *table, int32_t num_tensors, const void *chunks, int64_t num_chunks,
                           const float *partials, float max_norm, float *norm_out, void *stream);

#endif /* DFM_HIP_OPTIM_H */
