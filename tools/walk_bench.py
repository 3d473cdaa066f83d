#!/usr/bin/env python3
"""Device time of the greedy walk (k_walk.hip) at two shapes and K = 1, 256, 8192 random residue sequences on a resident mJ:
gdca_greedy_walk_dev with max_steps = 32 and with max_steps = 4 N (the mean walk length reported), the time per step and sequence,
against its floors per step -- two columns of 8 n bytes at the HBM rate k_fn20 reaches, and 2 N q LDS accesses of 8 bytes -- and
against what a caller had to do for one step before: gdca_mutation_scan_dev, a download of D, a numpy argmin over the admissible
entries and an upload of the changed sequences.  One process; the context is made before anything is timed; HIP events on the stream
the context works on for the device calls, the host clock around the old route's step (its host work is part of it); every GPU step
under a time limit of its own (a step that overruns ends the process with status 124, nothing is started after it).

    python tools/walk_bench.py --config B --out profiles/walk_bench.json   (N = 128, M = 10 000)
    python tools/walk_bench.py --config C --out profiles/walk_bench.json   (N = 500, M = 50 000)
Results of several configs are merged into one JSON file by config name."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")

from mutation_bench import CONFIGS, CUS, FN_HBM_FRACTION, GHZ, KS, LDS_BYTES_PER_CLK, PEAK_HBM, step_limit, timed  # noqa: E402

LINE = 128  # bytes one strided 8-byte read brings along (a cache line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--old-steps", type=int, default=5, help="timed steps of the old route (one more runs first, untimed)")
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, M, q, theta, pc = c["N"], c["M"], 21, c["theta"], args.pseudocount
    s = q - 1
    n = N * s
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    KMAX = max(KS)
    X = np.random.default_rng(c["seed"]).integers(1, q, size=(KMAX, N)).astype(np.int8)  # (K, N) rows = N x K column-major; residues only
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dX = torch.from_numpy(X).cuda()
        dD = torch.empty(KMAX * N * q, dtype=torch.float64, device="cuda")
        dXout = torch.empty((KMAX, N), dtype=torch.int8, device="cuda")
        dsteps = torch.empty(KMAX, dtype=torch.int32, device="cuda")
        dsum = torch.empty(KMAX, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, M=M, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats, warmup=args.warmup,
               old_route_steps=args.old_steps, sequences="uniformly random residues, no gaps", flags=0, min_gain=0.0, K={})

    # ---- the resident model (the library's own device operators on the synthetic family)
    with step_limit(180, "operator chain"):
        dPi = torch.empty(n, dtype=torch.float64, device="cuda")
        dmJ = torch.empty(n * n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dW, Meff, _, _ = devops.compute_weights_dev(ctx, dZ.data_ptr(), N, M, theta if theta >= 0 else ":auto")
        devops.compute_weighted_frequencies_dev(ctx, dZ.data_ptr(), N, M, q, dW, Meff, dPi.data_ptr(), dmJ.data_ptr())
        devops.add_pseudocount_dev(ctx, dPi.data_ptr(), dmJ.data_ptr(), N, q, pc)
        devops.compute_C_dev(ctx, dPi.data_ptr(), dmJ.data_ptr(), n, dC=dmJ.data_ptr())
        devops.inv_cholesky_dev(ctx, dmJ.data_ptr(), n)
        ctx.synchronize()

    def walk(K, T):
        ctx.greedy_walk_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), K, None, 0, 0.0, T, dXout.data_ptr(), dsteps.data_ptr(),
                            dsum.data_ptr())

    hbm_rate = [f * PEAK_HBM for f in FN_HBM_FRACTION]
    lds_rate = CUS * GHZ * 1e9 * LDS_BYTES_PER_CLK
    for K in KS:
        r = {}
        with step_limit(240, "scan K=%d" % K):
            ms = timed(lambda: ctx.mutation_scan_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), K, gd._lib.MUT_POTENTIAL, dD.data_ptr()),
                       args.warmup, args.repeats)
            r["scan_ms"] = statistics.median(ms)  # the walk's first stage, and the old route's device part
        for T, key in ((32, "walk32"), (4 * N, "walk4N")):
            with step_limit(600, "gdca_greedy_walk_dev K=%d max_steps=%d" % (K, T)):
                ms = timed(lambda: walk(K, T), args.warmup, args.repeats)
                steps = dsteps[:K].cpu().numpy().astype(np.int64)
            r[key + "_ms"] = statistics.median(ms)
            r[key + "_ms_all"] = ms
            r[key + "_max_steps"] = T
            r[key + "_mean_steps"] = float(steps.mean())
            r[key + "_longest"] = int(steps.max())
            r[key + "_cut_off"] = int((steps == T).sum())
            total = float(steps.sum())
            r[key + "_us_per_step_and_sequence"] = (r[key + "_ms"] - r["scan_ms"]) * 1e3 / total       # the walk kernel alone
            r[key + "_us_per_step_and_sequence_with_scan"] = r[key + "_ms"] * 1e3 / total
            r[key + "_ms_per_step"] = (r[key + "_ms"] - r["scan_ms"]) / float(steps.max())             # a step of the whole batch
        r["lds_table"] = bool(8 * (4 + N * q) + 32 + 2 * N <= 160 * 1024)

        # ---- floors of ONE step of the K sequences.  HBM: two columns of 8 n bytes a sequence at k_fn20's rate.  LDS: 2 N q accesses of
        # 8 bytes a sequence (the scan's two reads an entry; the update's read and write of the N s residue entries are within that count)
        r["floor_hbm_bytes_per_step"] = 16.0 * n * K
        r["floor_hbm_ms_per_step"] = [r["floor_hbm_bytes_per_step"] / f * 1e3 for f in hbm_rate]
        r["floor_lds_bytes_per_step"] = 16.0 * N * q * K
        # (one workgroup a sequence: K < compute units leaves the others' LDS idle)
        r["floor_lds_ms_per_step"] = r["floor_lds_bytes_per_step"] / (lds_rate * min(K, CUS) / CUS) * 1e3
        r["floor_ms_per_step"] = max(min(r["floor_hbm_ms_per_step"]), r["floor_lds_ms_per_step"])
        r["floor_binds"] = "hbm" if min(r["floor_hbm_ms_per_step"]) >= r["floor_lds_ms_per_step"] else "lds"
        r["floor_fraction_walk32"] = r["floor_ms_per_step"] / r["walk32_ms_per_step"]
        r["floor_fraction_walk4N"] = r["floor_ms_per_step"] / r["walk4N_ms_per_step"]
        # what the tiling moves (a model, not a counter): the rows below the column's diagonal element are contiguous (16 bytes a row for
        # the two columns), the rows above it a stride-ld walk: one line a row, shared by the two columns; the diagonal sits half way on average
        r["tiling_bytes_per_step"] = K * (n / 2.0 * 16.0 + n / 2.0 * LINE)

        # ---- the old route, one step: scan (delta), download, argmin on the host, upload of the changed sequences
        with step_limit(600, "old route K=%d" % K):
            Xh = X[:K].copy()
            dXo = torch.from_numpy(Xh).cuda()
            rows = np.arange(K)
            ts = []
            for it in range(args.old_steps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.mutation_scan_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dXo.data_ptr(), K, gd._lib.MUT_DELTA, dD.data_ptr())
                D = dD[:K * N * q].view(K, N, q).cpu().numpy()
                D[:, :, q - 1] = np.inf                                          # flags = 0: the gap is no target
                D[rows[:, None], np.arange(N)[None, :], Xh.astype(np.int64) - 1] = np.inf   # ... nor the own symbol
                code = D.reshape(K, N * q).argmin(axis=1)
                best = D.reshape(K, N * q)[rows, code]
                go = best < 0.0
                Xh[rows[go], code[go] // q] = (code[go] % q + 1).astype(np.int8)
                dXo.copy_(torch.from_numpy(Xh))
                torch.cuda.synchronize()
                if it:
                    ts.append((time.perf_counter() - t0) * 1e3)
            r["old_route_ms_per_step"] = statistics.median(ts)
            r["old_route_ms_per_step_all"] = ts
            del D
        r["speedup_per_step_walk32"] = r["old_route_ms_per_step"] / (r["walk32_ms"] / r["walk32_longest"])  # (the walk's scan included)
        r["speedup_per_step_walk4N"] = r["old_route_ms_per_step"] / (r["walk4N_ms"] / r["walk4N_longest"])
        r["walk_is_faster"] = bool(r["speedup_per_step_walk32"] > 1.0 and r["speedup_per_step_walk4N"] > 1.0)
        res["K"][str(K)] = r
        print("K %5d: walk32 %.3f ms, walk4N %.3f ms (mean %.1f steps), old route %.3f ms a step, speedup a step %.1f / %.1f" %
              (K, r["walk32_ms"], r["walk4N_ms"], r["walk4N_mean_steps"], r["old_route_ms_per_step"], r["speedup_per_step_walk32"],
               r["speedup_per_step_walk4N"]), flush=True)
    ctx.close()

    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[args.config] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(allres, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    assert all(v["walk_is_faster"] for v in res["K"].values()), "the walk must beat the old route at every measured size"


if __name__ == "__main__":
    main()
