"""Are the gfx950 kernels of two builds the same machine code?

    python tools/compare_isa.py OLD_OBJ_DIR NEW_OBJ_DIR

For every `hipcc -c` object of both directories (lib/obj of two checkouts built with the same hipcc) the code
object is disassembled (verify_async_asm.disassemble_object), cut per kernel symbol, and each kernel reduced to
a hash of its instructions -- mnemonics, operands and encodings, the address column dropped -- plus the
resources its entry in the code object's metadata note declares (register counts, LDS and scratch bytes, spill
counts, workgroup size).  Kernels are matched by NAME over the whole library, so a kernel that moved to another
translation unit compares equal; the report lists the kernels that moved, appeared, vanished or differ.  What a
source-only refactor has to print is "0 differ", nothing added and nothing removed.  Exit status 1 otherwise.
"""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_async_asm as vaa  # noqa: E402

READELF = os.path.join(os.path.dirname(vaa.OBJDUMP), 'llvm-readelf')
_LINE = re.compile(r'^\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:\s*(.*?)\s*$')
RESOURCES = ('.vgpr_count', '.sgpr_count', '.agpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
             '.vgpr_spill_count', '.sgpr_spill_count', '.max_flat_workgroup_size', '.kernarg_segment_size',
             '.wavefront_size', '.uses_dynamic_stack')


def kernel_hashes(text):
    """{symbol: (instruction count, sha1 of 'mnemonic operands | encoding' lines)} of a disassembly"""
    out, name, h, n = {}, None, None, 0
    for l in text.splitlines() + ['0 <end>:']:
        m = re.match(r'^[0-9a-fA-F]+ <(.*)>:\s*$', l)
        if m:
            if name is not None:
                out[name] = (n, h.hexdigest())
            name, h, n = m.group(1), hashlib.sha1(), 0
            continue
        m = _LINE.match(l)
        if m and name is not None:
            h.update(('%s | %s\n' % (m.group(1), m.group(2))).encode())
            n += 1
    return out


def kernel_resources(notes):
    """{kernel name: {resource: value}} from `llvm-readelf --notes` of a code object"""
    out, cur = {}, None
    for l in notes.splitlines():
        m = re.match(r'^  (- | {2})(\.\w+):\s*(.*?)\s*$', l)  # a key of an amdhsa.kernels entry (not of its .args)
        if not m:
            continue
        if m.group(1) == '- ':
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3).strip("'")
        if m.group(2) == '.name':
            out[cur['.name']] = cur
    return {k: tuple((r, v.get(r)) for r in RESOURCES) for k, v in out.items()}


def object_kernels(obj):
    """{kernel: (object, instructions, hash, resources)} of one object; device functions that are no kernels
    (no metadata entry) are left out"""
    tmp = tempfile.mkdtemp(prefix='dfm_isacmp_')
    try:
        local = os.path.join(tmp, os.path.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([vaa.OBJDUMP, '--offloading', local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       check=True, cwd=tmp)
        cos = [f for f in os.listdir(tmp) if 'amdgcn' in f]
        notes = subprocess.run([READELF, '--notes', os.path.join(tmp, cos[0])], stdout=subprocess.PIPE, check=True,
                               text=True).stdout if cos else ''
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if not cos:
        return {}
    hashes, res = kernel_hashes(vaa.disassemble_object(obj)), kernel_resources(notes)
    missing = [k for k in res if k not in hashes]
    if missing:
        raise RuntimeError('%s: metadata names kernels the disassembly lacks: %s' % (obj, missing[:3]))
    return {k: (os.path.basename(obj),) + hashes[k] + (res[k],) for k in res}


def library_kernels(obj_dir):
    """{kernel: {object: (instructions, hash, resources)}}: a kernel template of a shared header is instantiated
    in every object that launches it"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(obj_dir, '*.o'))):
        for k, v in object_kernels(obj).items():
            out.setdefault(k, {})[v[0]] = v[1:]
    return out


def main(old_dir, new_dir):
    old, new = library_kernels(old_dir), library_kernels(new_dir)
    removed, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    both = sorted(set(old) & set(new))
    differ = [k for k in both if set(old[k].values()) != set(new[k].values())]
    moved = [k for k in both if set(old[k]) != set(new[k])]
    count = lambda lib: sum(len(v) for v in lib.values())
    print('kernels: %d old, %d new (%d / %d instances over all objects)' % (len(old), len(new), count(old), count(new)))
    print('%d removed, %d added, %d differ (instructions + encodings, or metadata resources)' % (
        len(removed), len(added), len(differ)))
    for title, names in (('removed', removed), ('added', added), ('differ', differ)):
        for k in names:
            print('  %s: %s' % (title, k))
    print('%d in other objects than before:' % len(moved))
    for k in moved:
        print('  %s -> %s  %s' % (','.join(sorted(old[k])), ','.join(sorted(new[k])), k))
    return 1 if removed or added or differ else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
