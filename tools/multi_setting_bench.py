"""Several settings of one alignment: single calls against one gdca_run_multi call, in one process on one GPU.

Config C (gdca_synth_family N = 500, M = 50 000, q = 21: n = 10 000).  After a warm-up, REPS alternating repetitions of three cases,
each both device-resident (gdca_run_dev per setting against gdca_run_multi_dev) and from a FASTA file (gDCA per setting against
gDCA_multi):
    pair   0.8 frob + 0.2 DI
    same   0.2 frob + 0.2 DI          (one pseudocount: one inverse)
    scan   0.1, 0.2, 0.4, 0.6, 0.8 frob
Wall-clock time of the calls (all synchronous), median and spread over the repetitions; the multi call's outputs are checked equal
to the single calls' once.  The new kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script
(--reps 2 --no-file); --kernel-bytes prints the bytes it moves, for the fraction of HBM peak.

    python tools/multi_setting_bench.py [--reps 20] [--N 500 --M 50000] [--no-file] > profiles/multi_setting_bench.log
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (torch's HIP runtime first: INTEGRATION.md "load order")

import gaussdca.jl_amd as g  # noqa: E402
from gaussdca.jl_amd import synth  # noqa: E402

FROB, DI = 0, 1
CASES = {
    "pair": [(0.8, FROB), (0.2, DI)],
    "same": [(0.2, FROB), (0.2, DI)],
    "scan": [(0.1, FROB), (0.2, FROB), (0.4, FROB), (0.6, FROB), (0.8, FROB)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=500)
    ap.add_argument("--M", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-file", action="store_true", help="device-resident calls only")
    a = ap.parse_args()
    N, M, q = a.N, a.M, 21
    n = N * (q - 1)
    Zo = synth.synth_family(N, M, q, synth.SEEDS["C"])              # (M, N) == N x M column-major
    ctx = g.Context(0)
    ctx.set_timing(False)
    dZ = torch.from_numpy(Zo).cuda()
    K_max = max(len(s) for s in CASES.values())
    dS = torch.empty((K_max, N, N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    tmp = tempfile.mkdtemp(prefix="multi_bench_")
    fasta = os.path.join(tmp, "C.fasta")
    synth.write_fasta(fasta, Zo)

    def dev_single(settings):
        for k, (pc, sc) in enumerate(settings):
            ctx.run_dev(dZ.data_ptr(), N, M, q, pc, -1.0, sc, dS[k].data_ptr())

    def dev_multi(settings):
        ctx.run_multi_dev(dZ.data_ptr(), N, M, q, settings, -1.0, dS.data_ptr())

    def file_single(settings):
        return [g.gDCA(fasta, pseudocount=pc, score="DI" if sc == DI else "frob", ctx=ctx) for pc, sc in settings]

    def file_multi(settings):
        return g.gDCA_multi(fasta, [(pc, "DI" if sc == DI else "frob") for pc, sc in settings], ctx=ctx)

    # the outputs once: every multi member equal to its single call
    for name, settings in CASES.items():
        dev_single(settings)
        want = dS[:len(settings)].cpu().numpy().copy()
        dS.fill_(float("nan"))
        torch.cuda.synchronize()  # (torch's stream is not the context's)
        dev_multi(settings)
        got = dS[:len(settings)].cpu().numpy()
        same = all(np.array_equal(want[k], got[k]) for k in range(len(settings)))
        if not a.no_file:
            R1, Rm = file_single(settings), file_multi(settings)
            same = same and all(np.array_equal(x.score, y.score) and np.array_equal(x.i, y.i) for x, y in zip(R1, Rm))
        print("# %-4s %s: multi outputs equal to the single calls: %s" % (name, settings, same), flush=True)
        if not same:
            sys.exit(1)

    forms = [("dev", dev_single, dev_multi)] + ([] if a.no_file else [("file", file_single, file_multi)])
    t = {(c, f, w): [] for c in CASES for f, _, _ in forms for w in ("single", "multi")}
    for rep in range(a.warmup + a.reps):
        for name, settings in CASES.items():
            for f, single, multi in forms:
                order = (("single", single), ("multi", multi)) if rep % 2 == 0 else (("multi", multi), ("single", single))
                for w, fn in order:   # alternating which goes first
                    t0 = time.perf_counter()
                    fn(settings)
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep >= a.warmup:
                        t[(name, f, w)].append(dt)
    print("# config N=%d M=%d q=%d (n=%d), %d repetitions after %d warm-up, wall-clock ms per case (all calls synchronous)" % (N, M, q, n, a.reps, a.warmup))
    print("%-5s %-5s %12s %12s %12s %12s %8s" % ("case", "form", "single med", "single IQR", "multi med", "multi IQR", "ratio"))
    for name in CASES:
        for f, _, _ in forms:
            s, m = t[(name, f, "single")], t[(name, f, "multi")]
            qs, qm = statistics.quantiles(s, n=4), statistics.quantiles(m, n=4)
            print("%-5s %-5s %12.2f %12.2f %12.2f %12.2f %8.3f" % (name, f, statistics.median(s), qs[2] - qs[0], statistics.median(m), qm[2] - qm[0],
                                                                statistics.median(m) / statistics.median(s)), flush=True)
    print("# k_cov_from_pij moves 8 n^2 (Pij_true) + 8 n^2 (C) + 8 n (Pi') bytes = %.3f GB per launch at n = %d" % ((16.0 * n * n + 8.0 * n) / 1e9, n))
    ctx.close()
    os.remove(fasta)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
