"""Per-call timing of the stride-2 3x3 backward kernels (hip/convs2bwd.h)
against the aten.convolution_backward calls they replace, N=256, both
transition shapes.  Library side uses the in-repo tuned MIOpen db staged
the way bench.py stages it.  Device events over ITERS calls, REPS
alternating repeats so the run-to-run spread is visible.  Each case is
timed twice: eager launches (host dispatch included, what a plain loop
pays) and replay of a captured graph of GCALLS calls (device time only,
what GraphStepper pays).  `--prof` shrinks the run for a kernel trace."""
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
        _dst = '/tmp/ft_s2micro_%s_%d' % (_sub, os.getpid())
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


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / ITERS   # us per call


def graphed(fn):
    """one graph of GCALLS back-to-back calls; returns its replay"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GCALLS):
            fn()
    return g.replay


for Ci, Wi in ((16, 32), (32, 16)):
    Co = 2 * Ci
    x = torch.randn(N, Ci, Wi, Wi, device='cuda').to(
        memory_format=CL).bfloat16()
    dy = torch.randn(N, Co, Wi // 2, Wi // 2, device='cuda').to(
        memory_format=CL).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, device='cuda') / (9 * Ci) ** .5).to(
        memory_format=CL).bfloat16()

    def lib(mask):
        return lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, mask)

    def both():
        ops._C.conv3x3s2_dgrad(dy, w)
        ops._C.conv3x3s2_wrw(dy, x)

    cases = (
        ('hip dgrad', lambda: ops._C.conv3x3s2_dgrad(dy, w)),
        ('lib dgrad', lib([True, False, False])),
        ('hip wrw', lambda: ops._C.conv3x3s2_wrw(dy, x)),
        ('lib wrw', lib([False, True, False])),
        ('hip dgrad+wrw', both),
        ('lib combined', lib([True, True, False])),
    )
    for _name, fn in cases:
        for _ in range(WARM):
            fn()
    replays = [(name, graphed(fn)) for name, fn in cases]
    for _name, rp in replays:
        rp()
    for mode, runs, div in (('eager', cases, 1), ('graph', replays, GCALLS)):
        res = {name: [] for name, _ in runs}
        for _ in range(REPS):
            for name, fn in runs:
                res[name].append(timed(fn) / div)
        for name, _ in runs:
            v = res[name]
            print('Ci%-2d Wi%-2d %s %-14s %s us/call  (min %.1f max %.1f)' % (
                Ci, Wi, mode, name, ' '.join('%6.1f' % t for t in v),
                min(v), max(v)), flush=True)
print('S2BWD_MICRO_OK')
