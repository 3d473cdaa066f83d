#!/usr/bin/env python3
"""Device time of one pseudo-likelihood gradient (k_plm.hip with the mutation stage) at two shapes on a resident model, through the
operator forms: the scan alone (gdca_mutation_scan_dev over all M sequences), scan + softmax (gdca_plm_conditionals_dev: softmax = the
difference), the tally with its pack, fill and finish (gdca_plm_tally_dev on the resident p; the same call on ONE sequence is the
pack + fill + finish share), the fused gradient (gdca_plm_tallies_dev) and an iteration of the enqueued loop (gdca_plm_learn_dev).
The tally is held against three floors: the LDS read-modify-writes (one ds_read_b64 + ds_write_b64 a row, sequence and column site: 2 +
6 LDS cycles a wave), the L2 reads of p its shape implies (N / 4 column groups each read all of p; the shared-row rate), and the dense
alternative 2 M n^2 flop on the FP64 matrix pipe.  HIP events on the stream the context works on, medians of `repeats` after `warmup`.

    python tools/plm_bench.py --config B --out profiles/plm_bench.json   (N = 128, M = 10 000)
    python tools/plm_bench.py --config C --out profiles/plm_bench.json   (N = 500, M = 50 000)
    python tools/plm_bench.py --golden tests/golden/reference/large.fasta.gz --iters 200   (the fit of a real family, and what the
        sampler and the Boltzmann machine make of it)
Results of several runs are merged into one JSON file by name."""
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

from mutation_bench import CONFIGS, CUS, GHZ, step_limit, timed  # noqa: E402

RMW_CLK = 2 + 6                    # ds_read_b64 + ds_write_b64, LDS cycles a wave-instruction pair
L2_SHARED = (16.8e12, 18.8e12)     # bytes / s, rows shared by every workgroup
MFMA_F64 = 78.6e12                 # flop / s


def config(args):
    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import _lib, devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, M, q, theta = c["N"], c["M"], 21, c["theta"]
    s, n = q - 1, N * (q - 1)
    stream = torch.cuda.current_stream()
    with step_limit(60, "context"):
        ctx = gd.Context(0, stream=stream.cuda_stream)
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    f64 = dict(dtype=torch.float64, device="cuda")
    with step_limit(120, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dp = torch.empty(M * N * q, **f64)
        dnk, dzero, dnll, dtrace = torch.empty(M, **f64), torch.zeros(n, **f64), torch.empty(1, **f64), torch.empty(4 * 3, **f64)
        dPi_d, dPij_d, dPi_c, dPij_c = torch.empty(n, **f64), torch.empty(n * n, **f64), torch.empty(n, **f64), torch.empty(n * n, **f64)
        torch.cuda.synchronize()
    p = lambda t: t.data_ptr()  # noqa: E731
    with step_limit(180, "weights, frequencies, start"):
        dw, Meff, _, _ = devops.compute_weights_dev(ctx, p(dZ), N, M, theta if theta >= 0 else ":auto")
        devops.compute_weighted_frequencies_dev(ctx, p(dZ), N, M, q, dw, Meff, p(dPi_d), p(dPij_d))
        W0 = gd.potts_independent(np.maximum(dPi_d.cpu().numpy(), 1e-3) * 0.9, N, q)
        dW = torch.from_numpy(np.asfortranarray(W0)).cuda()
        ctx.synchronize()
    res = dict(config=args.config, N=N, M=M, q=q, n=n, Meff=Meff, repeats=args.repeats, warmup=args.warmup)
    med = statistics.median
    with step_limit(900, "stages"):
        ms_scan = timed(lambda: devops.mutation_scan_dev(ctx, p(dW), p(dzero), N, q, p(dZ), M, _lib.MUT_POTENTIAL, p(dp)), args.warmup, args.repeats)
        ms_cond = timed(lambda: devops.plm_conditionals_dev(ctx, p(dW), p(dZ), N, M, q, p(dp), p(dnk)), args.warmup, args.repeats)
        ms_tally = timed(lambda: devops.plm_tally_dev(ctx, p(dp), p(dZ), dw, Meff, N, M, q, p(dPi_c), p(dPij_c)), args.warmup, args.repeats)
        ms_fin = timed(lambda: devops.plm_tally_dev(ctx, p(dp), p(dZ), dw, Meff, N, 1, q, p(dPi_c), p(dPij_c)), args.warmup, args.repeats)
        ms_grad = timed(lambda: devops.plm_tallies_dev(ctx, p(dW), p(dZ), dw, Meff, N, M, q, p(dPi_c), p(dPij_c), p(dnll)), args.warmup,
                        args.repeats)
        ms_loop = timed(lambda: devops.plm_learn_dev(ctx, p(dW), p(dZ), dw, Meff, p(dPi_d), p(dPij_d), N, M, q, 3, 1.0 / N, 0.01, p(dtrace)),
                        1, 3)
    tally = med(ms_tally) - med(ms_fin)
    waves = (n + 63) // 64
    floors = dict(lds_ms=waves * M * N * RMW_CLK / (CUS * GHZ * 1e9) * 1e3,
                  l2_ms=[((N + 3) // 4) * 8.0 * M * N * q / r * 1e3 for r in L2_SHARED],
                  dense_mfma_ms=2.0 * M * n * n / MFMA_F64 * 1e3)
    res.update(scan_ms=med(ms_scan), scan_softmax_ms=med(ms_cond), softmax_ms=med(ms_cond) - med(ms_scan), tally_call_ms=med(ms_tally),
               pack_fill_finish_ms=med(ms_fin), tally_ms=tally, gradient_ms=med(ms_grad), loop_ms_per_iteration=med(ms_loop) / 3,
               all=dict(scan=ms_scan, cond=ms_cond, tally=ms_tally, fin=ms_fin, grad=ms_grad, loop3=ms_loop), floors=floors,
               tally_over_lds_floor=tally / floors["lds_ms"], tally_over_dense=tally / floors["dense_mfma_ms"])
    print("config %s: scan %.2f, softmax %.2f, tally %.2f (LDS floor %.2f, L2 floor %.2f, dense %.2f), pack+fill+finish %.2f, gradient %.2f, "
          "loop %.2f ms / iteration" % (args.config, res["scan_ms"], res["softmax_ms"], tally, floors["lds_ms"], floors["l2_ms"][1],
                                        floors["dense_mfma_ms"], res["pack_fill_finish_ms"], res["gradient_ms"],
                                        res["loop_ms_per_iteration"]), flush=True)
    return "config_" + args.config, res


def golden(args):
    import gaussdca.jl_amd as gd

    name = os.path.basename(args.golden).split(".")[0]
    Z = gd.read_fasta_alignment(args.golden, 0.9)
    N, q = Z.shape[0], int(Z.max())
    rows = sorted(set(list(range(0, args.iters, 20)) + [args.iters - 1]))
    with step_limit(300, "gDCA"):
        top = [(i, j) for i, j, _ in gd.gDCA(args.golden)[:N]]
    res = dict(file=os.path.basename(args.golden), N=N, q=q, M=int(Z.shape[1]), iters=args.iters, lam=args.lam, trace_rows=rows,
               columns=["max |Pi_c - Pi_d|", "max |c_c - c_d|", "pearson", "nll"])
    fits = {}
    for adapt in (False, True):
        with step_limit(900, "gDCA_plm adapt=%s" % adapt):
            t0 = time.perf_counter()
            W, trace, R = gd.gDCA_plm(args.golden, args.iters, lam=args.lam, adapt=adapt, scores=True)
            dt = time.perf_counter() - t0
        mine = set((i, j) for i, j, _ in R[:N])
        fits[adapt] = W
        res["adapt" if adapt else "default_step"] = dict(seconds=dt, trace=[trace[r].tolist() for r in rows], finite=bool(np.isfinite(W).all()),
                                                         top_N_overlap_with_gaussian=len(mine & set(top)) / float(N))
        print("adapt=%s: %.1f s, nll %.4f -> %.4f, top-N overlap %.3f" % (adapt, dt, trace[0, 3], trace[-1, 3],
                                                                           res["adapt" if adapt else "default_step"]["top_N_overlap_with_gaussian"]),
              flush=True)
    # the sampler under the plm model: acceptance at beta = 1 from the family's first sequences
    K = min(1024, Z.shape[1])
    X = np.asfortranarray(Z[:, :K])
    for key, W in (("default_step", fits[False]), ("adapt", fits[True])):
        with step_limit(300, "sample"):
            out = gd.sample(W, np.zeros(W.shape[0]), X, q, beta=1.0, burn=10 * N, stride=N, n_samples=1, seed=1, gaps=True)
        acc = np.asarray(out[2], dtype=np.float64)  # (Xs, dE_s, accepted)
        res[key]["acceptance_beta1"] = float(acc.sum() / (K * 11.0 * N))
        print("%s: acceptance at beta = 1: %.4f" % (key, res[key]["acceptance_beta1"]), flush=True)
    with step_limit(900, "gDCA_bm init=plm"):
        Wb, tb = gd.gDCA_bm(args.golden, 40, K=1024, init="plm", plm_iter=args.iters, plm_lam=args.lam, seed=1)
    res["bm_init_plm"] = dict(columns=["max |Pi_m - Pi_d|", "max |c_m - c_d|", "pearson", "acceptance"], trace=tb.tolist())
    print("gDCA_bm(init=plm): first / last rows %s %s" % (tb[0].tolist(), tb[-1].tolist()), flush=True)
    return "golden_" + name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--golden")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--lam", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plm_bench.json"))
    args = ap.parse_args()
    key, res = golden(args) if args.golden else config(args)
    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[key] = res
    with open(args.out, "w") as f:
        json.dump(allres, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
