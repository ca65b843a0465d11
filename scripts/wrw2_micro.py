"""Per-call timing of the 3x3/stride-1 weight gradient conv3x3_wrw2
(hip/convwrw2.h: main kernel + one final kernel) against the library's
wrw-only aten.convolution_backward call (its SubTensorOp/cast wrapper
kernels included), N=256, the three body shapes.  Library side uses the
in-repo tuned MIOpen db staged the way bench.py stages it.  Device events
over ITERS calls of a replayed graph of GCALLS back-to-back calls (device
time only: what a GraphStepper step pays), REPS alternating repeats so the
run-to-run spread is visible.

  --sweep   hip only: time every stream cap in SWEEP through FT_WRW2_NBLK
            (the launcher reads it per call; a graph keeps the cap it was
            captured with)
  --hip     hip only at the default caps (e.g. to time another build)
  --prof    shrink the run for a kernel trace"""
import os
import shutil
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault('MIOPEN_FIND_MODE', '2')
_MDB = os.path.join(REPO, 'fedtorch_amd', 'miopen_db')
for _sub, _var in (('udb', 'MIOPEN_USER_DB_PATH'),
                   ('cache', 'MIOPEN_CUSTOM_CACHE_DIR')):
    _src = os.path.join(_MDB, _sub)
    if os.path.isdir(_src):
        _dst = '/tmp/ft_wrw2micro_%s_%d' % (_sub, os.getpid())
        shutil.copytree(_src, _dst, dirs_exist_ok=True,
                        copy_function=shutil.copyfile)
        for _root, _, _ in os.walk(_dst):
            os.chmod(_root, 0o755)
        os.environ.setdefault(_var, _dst)

import torch  # noqa: E402
import fedtorch_amd.ops as ops  # noqa: E402

CL = torch.channels_last
N, WARM, ITERS, REPS, GCALLS = 256, 30, 300, 3, 20
if '--prof' in sys.argv:
    WARM, ITERS, REPS = 5, 20, 1
SHAPES = ((16, 32), (32, 16), (64, 8))
# stream caps: partial bytes = streams * 36*C*C, from ~2 MB up to the
# pre-diet 1024-block grid
SWEEP = {16: (256, 384, 512, 768, 1024),
         32: (64, 96, 128, 192, 256, 384, 512),
         64: (24, 32, 48, 64, 96, 128)}


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS // GCALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / ITERS   # us per call


def graphed(fn):
    """one graph of GCALLS back-to-back calls; returns its replay"""
    for _ in range(WARM):
        fn()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GCALLS):
            fn()
    g.replay()
    return g.replay


def report(C, runs):
    res = {name: [] for name, _ in runs}
    for _ in range(REPS):
        for name, fn in runs:
            res[name].append(timed(fn))
    for name, _ in runs:
        v = res[name]
        print('C%-2d graph %-22s %s us/call  (min %.1f max %.1f)' % (
            C, name, ' '.join('%6.1f' % t for t in v), min(v), max(v)),
            flush=True)


for C, W in SHAPES:
    x = torch.randn(N, C, W, W, device='cuda').to(
        memory_format=CL).bfloat16()
    dy = torch.randn(N, C, W, W, device='cuda').to(
        memory_format=CL).bfloat16()
    w = (torch.randn(C, C, 3, 3, device='cuda') / (9 * C) ** .5).to(
        memory_format=CL).bfloat16()

    def hip():
        return ops._C.conv3x3_wrw2(dy, x)

    def lib():
        return torch.ops.aten.convolution_backward(
            dy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
            [False, True, False])

    if '--sweep' in sys.argv:
        runs = []
        for cap in SWEEP[C]:
            os.environ['FT_WRW2_NBLK'] = str(cap)
            runs.append(('hip streams=%d' % cap, graphed(hip)))
        del os.environ['FT_WRW2_NBLK']
    elif '--hip' in sys.argv:
        runs = [('hip wrw (main+final)', graphed(hip))]
    else:
        runs = [('hip wrw (main+final)', graphed(hip)),
                ('lib wrw incl. wrappers', graphed(lib))]
    report(C, runs)
print('WRW2_MICRO_OK')
