#!/usr/bin/env python3
"""Device time of one Boltzmann-machine iteration (k_bm.hip with the sample and tally stages) at two shapes and K = 256, 8192 chains
on a resident model: the stages one by one through the operator forms -- the scan (gdca_mutation_scan_dev), the chains
(gdca_sample_dev minus the scan), the tally (gdca_frequencies_dev), the read-out, the update --, the enqueued loop (gdca_bm_learn_dev,
ms per iteration), and the "old route": the same five steps driven from Python with a download of the four trace numbers per
iteration.  The update kernel is held against its HBM floor of 32 n^2 bytes at the rate k_fn20 reaches on the same matrix.  An
iteration is one sweep of burn-in and one sample a sweep later (2 N proposals a chain).  One process; HIP events on the stream the
context works on for the device calls, the host clock around the old route; every GPU step under a time limit of its own.

    python tools/bm_bench.py --config B --out profiles/bm_bench.json   (N = 128, M = 10 000)
    python tools/bm_bench.py --config C --out profiles/bm_bench.json   (N = 500, M = 50 000)
    python tools/bm_bench.py --golden tests/golden/reference/large.fasta.gz --iters 100   (the trace of one run on a real family)
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

from mutation_bench import CONFIGS, FN_HBM_FRACTION, PEAK_HBM, step_limit, timed  # noqa: E402

KS = (256, 8192)


def golden(args):
    import gaussdca.jl_amd as gd

    with step_limit(900, "gDCA_bm on %s" % args.golden):
        t0 = time.perf_counter()
        W, trace = gd.gDCA_bm(args.golden, args.iters, K=args.chains, eta=args.eta, burn=args.burn, stride=args.stride, seed=1,
                              target_pseudocount=args.target_pseudocount)
        dt = time.perf_counter() - t0
    n = W.shape[0]
    rows = sorted(set(list(range(0, args.iters, max(args.iters // 10, 1))) + [args.iters - 1]))
    res = dict(file=os.path.basename(args.golden), n=n, iters=args.iters, K=args.chains, eta=args.eta, burn=args.burn, stride=args.stride,
               target_pseudocount=args.target_pseudocount, seconds=dt, columns=["max |Pi_m - Pi_d|", "max |c_m - c_d|", "pearson", "acceptance"],
               trace_rows=rows, trace=[trace[r].tolist() for r in rows], symmetric=bool(np.array_equal(W, W.T)), finite=bool(np.isfinite(W).all()))
    return "golden_" + os.path.basename(args.golden).split(".")[0], res


def config(args):
    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, M, q, theta, pc = c["N"], c["M"], 21, c["theta"], args.pseudocount
    n = N * (q - 1)
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    KMAX = max(KS)
    assert KMAX <= M
    f64 = dict(dtype=torch.float64, device="cuda")
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dX = torch.empty((KMAX, N), dtype=torch.int8, device="cuda")
        dXs = torch.empty((KMAX, N), dtype=torch.int8, device="cuda")
        dacc = torch.empty(KMAX, dtype=torch.int32, device="cuda")
        dV = torch.empty(KMAX * N * q, **f64)
        dones = torch.ones(KMAX, **f64)
        dzero = torch.zeros(n, **f64)
        dPi_d, dPij_d, dPi_m, dPij_m = torch.empty(n, **f64), torch.empty(n * n, **f64), torch.empty(n, **f64), torch.empty(n * n, **f64)
        dPi, dmJ, dWm = torch.empty(n, **f64), torch.empty(n * n, **f64), torch.empty(n * n, **f64)
        dout, dtrace = torch.empty(4, **f64), torch.empty(4 * args.iters, **f64)
        torch.cuda.synchronize()
    p = lambda t: t.data_ptr()  # noqa: E731
    res = dict(config=args.config, N=N, M=M, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats, warmup=args.warmup, burn=N, stride=N,
               n_samples=1, loop_iters=args.iters, K={})

    with step_limit(180, "operator chain"):
        dWt, Meff, _, _ = devops.compute_weights_dev(ctx, p(dZ), N, M, theta if theta >= 0 else ":auto")
        devops.compute_weighted_frequencies_dev(ctx, p(dZ), N, M, q, dWt, Meff, p(dPi_d), p(dPij_d))  # the target: pseudocount 0
        devops.add_pseudocount_dev(ctx, p(dPi_d), p(dPij_d), N, q, pc, p(dPi), p(dmJ))
        devops.compute_C_dev(ctx, p(dPi), p(dmJ), n, dC=p(dmJ))
        devops.inv_cholesky_dev(ctx, p(dmJ), n)
        ms_start = timed(lambda: devops.potts_from_gaussian_dev(ctx, p(dmJ), p(dPi), N, q, p(dWm)), 1, 3)
        ctx.synchronize()
    res["potts_from_gaussian_ms"] = statistics.median(ms_start)

    # ---- the update against its floor
    floor = [32.0 * n * n / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]
    with step_limit(120, "update"):
        devops.compute_weighted_frequencies_dev(ctx, p(dZ), N, KMAX, q, p(dones), float(KMAX), p(dPi_m), p(dPij_m))
        ms = timed(lambda: devops.bm_update_dev(ctx, p(dWm), p(dPij_d), p(dPij_m), N, q, 1e-6, 0.0), args.warmup, args.repeats)
        ms_l2 = timed(lambda: devops.bm_update_dev(ctx, p(dWm), p(dPij_d), p(dPij_m), N, q, 1e-6, 0.01), args.warmup, args.repeats)
        ms_ro = timed(lambda: devops.bm_readout_dev(ctx, p(dPi_d), p(dPij_d), p(dPi_m), p(dPij_m), N, q, p(dout)), args.warmup, args.repeats)
    upd = statistics.median(ms)
    res["update"] = dict(ms=upd, ms_all=ms, ms_with_l2=statistics.median(ms_l2), bytes=32.0 * n * n, gb_per_s=32.0 * n * n / upd / 1e6,
                         fraction_of_peak=32.0 * n * n / upd / 1e-3 / PEAK_HBM, floor_ms=floor, floor_fraction=[f / upd for f in floor])
    res["readout"] = dict(ms=statistics.median(ms_ro), ms_all=ms_ro, bytes=8.0 * n * n)
    print("update %.3f ms (%.0f GB/s, floor %.3f .. %.3f ms), read-out %.3f ms" % (upd, res["update"]["gb_per_s"], floor[1], floor[0],
                                                                                    res["readout"]["ms"]), flush=True)

    for K in KS:
        r = {}
        T = 2 * N

        def reset():
            devops.potts_from_gaussian_dev(ctx, p(dmJ), p(dPi), N, q, p(dWm))
            dX[:K].copy_(dZ[:K])

        def one(t, download):
            ctx.sample_dev(p(dWm), p(dzero), N, q, p(dX), K, None, 1, 1.0, 1, t * K, N, N, 1, p(dXs), p(dacc))
            dX[:K].copy_(dXs[:K])
            devops.compute_weighted_frequencies_dev(ctx, p(dXs), N, K, q, p(dones), float(K), p(dPi_m), p(dPij_m))
            devops.bm_readout_dev(ctx, p(dPi_d), p(dPij_d), p(dPi_m), p(dPij_m), N, q, p(dout))
            devops.bm_update_dev(ctx, p(dWm), p(dPij_d), p(dPij_m), N, q, args.eta, 0.0)
            if download:
                out = dout.cpu().numpy()
                out[3] = float(dacc[:K].sum().item()) / (K * T)
                return out

        with step_limit(300, "stages K=%d" % K):
            reset()
            scan = timed(lambda: ctx.mutation_scan_dev(p(dWm), p(dzero), N, q, p(dX), K, gd._lib.MUT_POTENTIAL, p(dV)), args.warmup, args.repeats)
            samp = timed(lambda: ctx.sample_dev(p(dWm), p(dzero), N, q, p(dX), K, None, 1, 1.0, 1, 0, N, N, 1, p(dXs), p(dacc)), args.warmup,
                         args.repeats)
            tally = timed(lambda: devops.compute_weighted_frequencies_dev(ctx, p(dXs), N, K, q, p(dones), float(K), p(dPi_m), p(dPij_m)),
                          args.warmup, args.repeats)
            acc = float(dacc[:K].sum().item()) / (K * T)
        r["scan_ms"], r["chains_ms"] = statistics.median(scan), statistics.median(samp) - statistics.median(scan)
        r["tally_ms"], r["readout_update_ms"] = statistics.median(tally), res["readout"]["ms"] + upd
        r["stages_sum_ms"] = r["scan_ms"] + r["chains_ms"] + r["tally_ms"] + r["readout_update_ms"]
        r["acceptance_first_iteration"] = acc
        with step_limit(600, "loop K=%d" % K):
            def loop():
                reset()
                ctx.bm_learn_dev(p(dWm), p(dPi_d), p(dPij_d), N, q, p(dX), K, None, 1, 1.0, 1, 0, args.iters, N, N, 1, args.eta, 0.0, p(dtrace))
            ms = timed(loop, 1, 3)
            ms_reset = timed(reset, 1, 3)
            trace = dtrace.cpu().numpy().reshape(args.iters, 4)
        r["loop_ms_per_iteration"] = (statistics.median(ms) - statistics.median(ms_reset)) / args.iters
        r["loop_ms_all"], r["loop_trace_last"] = ms, trace[-1].tolist()
        with step_limit(600, "old route K=%d" % K):
            # the same iterations 0 .. iters - 1 from the same start as the loop, so that the two cost the same device work (an
            # iteration's cost follows the acceptance rate, which moves with the model); one untimed pass first
            ts = []
            for rep in range(3):
                reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for it in range(args.iters):
                    last = one(it, True)
                torch.cuda.synchronize()
                if rep:
                    ts.append((time.perf_counter() - t0) * 1e3 / args.iters)
        r["old_route_ms_per_iteration"], r["old_route_ms_all"], r["old_route_trace_last"] = statistics.median(ts), ts, last.tolist()
        r["old_route_equals_loop"] = bool(np.array_equal(last, trace[-1]))
        r["loop_speedup"] = r["old_route_ms_per_iteration"] / r["loop_ms_per_iteration"]
        res["K"][str(K)] = r
        print("K %5d: scan %.3f, chains %.3f, tally %.3f, read-out + update %.3f ms; loop %.3f ms an iteration, old route %.3f (x %.2f)" %
              (K, r["scan_ms"], r["chains_ms"], r["tally_ms"], r["readout_update_ms"], r["loop_ms_per_iteration"],
               r["old_route_ms_per_iteration"], r["loop_speedup"]), flush=True)
    ctx.close()
    return args.config, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C", choices=sorted(CONFIGS))
    ap.add_argument("--golden", default=None, help="a FASTA file: the trace of one gDCA_bm run instead of the timings")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10, help="iterations of the timed loop / of the golden run")
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--eta", type=float, default=1.0)
    ap.add_argument("--burn", type=int, default=None)
    ap.add_argument("--stride", type=int, default=None)
    ap.add_argument("--target-pseudocount", type=float, default=0.0)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"
    key, res = golden(args) if args.golden else config(args)
    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[key] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(allres, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
