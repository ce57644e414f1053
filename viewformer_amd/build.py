"""Build libvf_hip.so (gfx950) in-tree with hipcc.  ``python -m viewformer_amd.build [--force]``.

hipcc cross-compiles without a GPU; the resulting .so sits next to this file so that it
travels to the GPU box with the repo snapshot (it is git-ignored, not gpurun-ignored).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libvf_hip.so')
ARCH = 'gfx950'
# per-source extra flags.  -fno-slp-vectorize: the SLP vectoriser turns the fp32 prologue math into v_pk_*_f32, which costs MFMA issue slots
# beside the matrix instructions (MI355X guide, 'price of one filler'); measured +0.3 ... +0.9 % on the dominant kernel without it
EXTRA_FLAGS = {'conv3_halo_x3h': ['-fno-slp-vectorize']}


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.hip'))


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
    deps.append(os.path.join(os.path.dirname(HERE), 'include', 'vf_hip.h'))
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return LIB
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, 'build'), exist_ok=True)
    stems = {os.path.basename(s)[:-4] for s in sources()}
    for f in os.listdir(os.path.join(HERE, 'build')):              # objects of sources that have left csrc/ must not linger
        if f.endswith('.o') and f[:-2] not in stems:
            os.remove(os.path.join(HERE, 'build', f))
    for src in sources():
        obj = os.path.join(HERE, 'build', os.path.basename(src)[:-4] + '.o')
        cmd = [hipcc, f'--offload-arch={ARCH}', '-O3', '-std=c++17', '-fPIC', '-c', src, '-o', obj,
               '-Wall', '-Wno-unused-function'] + EXTRA_FLAGS.get(os.path.basename(src)[:-4], [])
        if verbose:
            cmd.append('-Rpass-analysis=kernel-resource-usage')
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    failed = False
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0 or verbose:
            sys.stderr.write(f'--- {os.path.basename(src)}\n{out}\n')
        failed |= p.returncode != 0
    if failed:
        raise RuntimeError('hipcc failed')
    cmd = [hipcc, f'--offload-arch={ARCH}', '-shared', '-fPIC', '-o', LIB] + objs
    subprocess.check_call(cmd)
    return LIB


# side-by-side builds of the same ABI that tests load next to the product library (never the product): name -> (extra flags, source stems)
VARIANTS = {
    # the transposing LDS reads of the DMA-ring kernels through the compiler intrinsic again instead of inline asm (vf_common.h: vf_tr_frag2_wait):
    # hipcc then orders them behind the ring with its own `s_waitcnt vmcnt(0)` — the slow but compiler-ordered reference of
    # tests/test_hip_ring_stress.py, which compares the two builds' results bit for bit
    'trintrin': (['-DVF_X_TRINTRIN'], ['attention_dma', 'attention_train_bf16', 'gemm_tn_bf16']),
}


def variant_path(name: str) -> str:
    return os.path.join(HERE, 'variants', f'libvf_{name}.so')


def build_variant(name: str, force: bool = False) -> str:
    """libvf_<name>.so under viewformer_amd/variants/: the product objects, with the variant's sources recompiled under its flags"""
    flags, stems = VARIANTS[name]
    build()
    out = variant_path(name)
    srcs = [os.path.join(CSRC, st + '.hip') for st in stems]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in srcs + hdrs + [LIB]):
        return out
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    procs, vobjs = [], []
    for st, src in zip(stems, srcs):
        obj = os.path.join(HERE, 'variants', f'{st}.{name}.o')
        cmd = [hipcc, f'--offload-arch={ARCH}', '-O3', '-std=c++17', '-fPIC', '-w', '-c', src, '-o', obj] + EXTRA_FLAGS.get(st, []) + flags
        procs.append(subprocess.Popen(cmd))
        vobjs.append(obj)
    if any(p.wait() != 0 for p in procs):
        raise RuntimeError(f'hipcc failed on variant {name}')
    objs = [os.path.join(HERE, 'build', os.path.basename(s)[:-4] + '.o') for s in sources() if os.path.basename(s)[:-4] not in stems]
    subprocess.check_call([hipcc, f'--offload-arch={ARCH}', '-shared', '-fPIC', '-o', out] + objs + vobjs)
    return out


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose='-v' in sys.argv))
