"""Where a tile of the consensus product (k_hamming_fp4) spends its time: shader-clock stamps of one lane of eight workgroups, from a
library built with -DGDCA_F4_STAMPS (tools/build_variant.sh stamps -DGDCA_F4_STAMPS; run with GDCA_LIB=<that library>).
usage: fp4_stamps.py [N [M]]   (default: config C, N = 500, M = 50 000)
Prints, per stamped workgroup and as the mean over them, a tile's clocks and their shares: "mfma" (top of the chunk -> MFMAs done;
it holds the issue of the next chunk's loads and of the flush's atomic), the LDS stores (the wait for those loads), the flush of the
tile before (wave 0: the wait for its atomic, the list's stores), the epilogue, the barrier."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussdca.jl_amd as g
from gaussdca.jl_amd import devops, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 500
M = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
WG, IT, PH = 8, 32, 10
ctx = g.Context(0)
fn = getattr(ctx.lib, "gdca_fp4_stamps", None)
if fn is None:
    sys.exit("this library was not built with -DGDCA_F4_STAMPS")
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
Z = synth.synth_family(N, M, 21, 7 + N)  # (M, N) row-major = N x M column-major
dZ = g.DeviceBuffer.from_array(ctx, np.ascontiguousarray(Z))
ctx.set_option("HAMMING_MODE", "mfma")
for _ in range(3):  # (the last launch's stamps stay)
    assert fn(None, 1) == 0
    devops.compute_weights_dev(ctx, dZ, N, M, 0.3)
    ctx.synchronize()
st = np.zeros(WG * IT * PH, dtype=np.int64)
assert fn(C.c_void_p(st.ctypes.data), 0) == 0
st = st.reshape(WG, IT, PH)
names = ("mfma (+ load issue)", "lds stores (load wait)", "flush", "epilogue", "barrier")
rows = []
for w in range(WG):
    its = [i for i in range(IT) if st[w, i, 0] and st[w, i, 5]]
    if len(its) < 3:
        continue
    its = its[1:]  # (the first chunk of the walk: waited for with nothing to do)
    mf = sum(st[w, i, 1] - st[w, i, 0] for i in its)
    ld = sum(st[w, i, 2] - st[w, i, 1] for i in its)
    fl = sum(st[w, i, 7] - st[w, i, 6] for i in its if st[w, i, 6])
    ep = sum(st[w, i, 4] - st[w, i, 3] for i in its if st[w, i, 3])
    ba = sum(st[w, i, 5] - max(st[w, i, 2], st[w, i, 4], st[w, i, 7]) for i in its)
    scan = sum(st[w, i, 8] - st[w, i, 3] for i in its if st[w, i, 3])
    take = sum(st[w, i, 9] - st[w, i, 8] for i in its if st[w, i, 9])
    tiles = sum(1 for i in its if st[w, i, 3])
    tot = st[w, its[-1], 5] - st[w, its[0], 0]
    rows.append((w, len(its), tiles, tot, mf, ld, fl, ep, ba))
    print("wg row %3d: %2d chunks %d tiles, %7d clocks = %6.0f a tile; " % (16 * w, len(its), tiles, tot, tot / max(tiles, 1)) +
          "  ".join("%s %.3f" % (n, v / tot) for n, v in zip(names, (mf, ld, fl, ep, ba))) +
          "  (of the epilogue: scan %.3f, prefix sum and LDS atomic %.3f)" % (scan / tot, take / tot))
if rows:
    a = np.array(rows, dtype=np.float64)
    tot = a[:, 3].sum()
    print("N %d M %d mean: %.0f clocks a tile; " % (N, M, tot / a[:, 2].sum()) +
          "  ".join("%s %.3f" % (n, a[:, 4 + k].sum() / tot) for k, n in enumerate(names)))
