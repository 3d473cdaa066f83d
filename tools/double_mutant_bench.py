#!/usr/bin/env python3
"""Device time of the double-mutant scan (k_epistasis.hip) at two shapes and K = 1, 256, 2048 backgrounds on a resident mJ: the map
stage (gdca_double_mutant_scan_dev: pack, g, the single-substitution scan, the map kernel) with the single-substitution scan's share
(gdca_mutation_scan_dev on the same sequences), the list form at L = 10^6 records (gdca_double_mutants_dev), against its two floors
(HBM and f64 VALU), against route (a), the only one the library had before -- gdca_energies_dev on the q^2 explicit double mutants of
ONE site pair of ONE sequence, SCALED to all N (N - 1) / 2 pairs and K sequences (building and uploading the mutants not included) --
and against route (b), a torch f64 formulation on the same GPU (the padded blocks gathered, broadcast-added, amin / argmin / norm)
for ONE sequence given the library's dE, SCALED by K (the N^2 q^2 tensor of one sequence is 0.9 GB at N = 500).  One process; the
context is made before anything is timed; HIP events on the stream the context works on; every GPU step under a time limit of its
own (a step that overruns ends the process with status 124, nothing is started after it).

    python tools/double_mutant_bench.py --config B --out profiles/double_mutant_bench.json   (N = 128, M = 10 000)
    python tools/double_mutant_bench.py --config C --out profiles/double_mutant_bench.json   (N = 500, M = 50 000)
Results of several configs are merged into one JSON file by config name."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")

CONFIGS = {"B": dict(N=128, M=10000, theta=0.2, seed=0xB128), "C": dict(N=500, M=50000, theta=-1.0, seed=0xC500)}
KS = (1, 256, 2048)
L_LIST = 1000000
PEAK_HBM = 8.0e12                  # bytes / s
FN_HBM_FRACTION = (0.58, 0.64)     # what k_fn20 reaches streaming the same matrix
CUS, GHZ, F64_LANES_PER_CLK = 256, 2.4, 64  # a compute unit issues 64 f64 add / mul lanes a clock (four SIMDs of 16)
OPS_PER_EVALUATION = 6             # four add / sub, the square, its addition (the compare-select not counted)
CHUNK = 64                         # sequences a workgroup of the map kernel


@contextlib.contextmanager
def step_limit(seconds, what):
    def over():
        sys.stderr.write("double_mutant_bench: step '%s' exceeded %d s\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    t = threading.Timer(seconds, over)
    t.daemon = True
    t.start()
    try:
        yield
    finally:
        t.cancel()


def timed(fn, warmup, repeats):
    """HIP events on the current torch stream (the context was made on it) -> list of ms"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "double_mutant_bench.json"))
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
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dX = dZ[:KMAX].contiguous()  # N x K column-major: the first K sequences of the family
        dEmin = torch.empty(KMAX * N * N, dtype=torch.float64, device="cuda")
        dcode = torch.empty(KMAX * N * N, dtype=torch.int32, device="cuda")
        depi = torch.empty(KMAX * N * N, dtype=torch.float64, device="cuda")
        dD = torch.empty(KMAX * N * q, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, M=M, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats, torch_repeats=args.torch_repeats,
               K={})

    # ---- a resident mJ (built by the library's own device operators)
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
    ptr = lambda t: t.data_ptr()  # noqa: E731

    # ---- route (a): gdca_energies_dev on the q^2 explicit double mutants of one site pair of one sequence (+ the wild type)
    with step_limit(180, "explicit double mutants"):
        x = dX[0]
        i0, j0 = 1, N - 2
        mut = x[None, :].repeat(q * q, 1)                                   # (q^2, N): mutant (b - 1) + q (c - 1)
        codes = torch.arange(q * q, device="cuda")
        mut[:, i0] = (codes % q + 1).to(torch.int8)
        mut[:, j0] = (codes // q + 1).to(torch.int8)
        mut = torch.cat([mut, x[None, :]], dim=0).contiguous()
        dEm = torch.empty(q * q + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ms = timed(lambda: ctx.energies_dev(ptr(dmJ), ptr(dPi), N, q, ptr(mut), q * q + 1, ptr(dEm)), args.warmup, args.repeats)
        res["mutants_one_pair_ms"] = statistics.median(ms)
        res["mutants_one_pair_ms_all"] = ms
        res["mutants_note"] = "gdca_energies_dev on the q^2 double mutants of ONE site pair of ONE sequence and the sequence itself; the " \
                              "per-K figures are this time SCALED by N (N - 1) / 2 pairs and K; building and uploading the mutants is not included"
        ddE_mut = (dEm[:-1] - dEm[-1]).clone()

    mJ = dmJ.view(n, n)
    for K in KS:
        r = {}
        with step_limit(300, "gdca_double_mutant_scan_dev K=%d" % K):
            ms = timed(lambda: ctx.double_mutant_scan_dev(ptr(dmJ), ptr(dPi), N, q, ptr(dX), K, ptr(dEmin), ptr(dcode), ptr(depi)), args.warmup,
                       args.repeats)
            r["maps_stage_ms"] = statistics.median(ms)
            r["maps_stage_ms_all"] = ms
            ms = timed(lambda: ctx.double_mutant_scan_dev(ptr(dmJ), ptr(dPi), N, q, ptr(dX), K, ptr(dEmin), None, None), args.warmup, args.repeats)
            r["maps_stage_emin_only_ms"] = statistics.median(ms)
            ms = timed(lambda: ctx.mutation_scan_dev(ptr(dmJ), ptr(dPi), N, q, ptr(dX), K, gd._lib.MUT_DELTA, ptr(dD)), args.warmup, args.repeats)
            r["single_scan_ms"] = statistics.median(ms)
            r["single_scan_ms_all"] = ms
            r["single_scan_share"] = r["single_scan_ms"] / r["maps_stage_ms"]
            r["map_kernel_ms"] = r["maps_stage_ms"] - r["single_scan_ms"]
            # the explicit mutants of route (a) against the map of sequence 0 at that pair
            ctx.double_mutant_scan_dev(ptr(dmJ), ptr(dPi), N, q, ptr(dX), K, ptr(dEmin), ptr(dcode), ptr(depi))
            torch.cuda.synchronize()
            adm = (mut[:-1, i0] != x[i0]) & (mut[:-1, j0] != x[j0])
            ref_min = float(ddE_mut[adm].min())
            r["mutants_vs_map_abs_over_scale"] = abs(float(dEmin[i0 + N * j0]) - ref_min) / float(ddE_mut.abs().max())
        with step_limit(300, "gdca_run_double_mutant_scan_dev K=%d" % K):
            sts = []
            for it in range(args.warmup + args.repeats):
                st = ctx.run_double_mutant_scan_dev(ptr(dZ), N, M, q, pc, theta, ptr(dX), K, ptr(dEmin), ptr(dcode), ptr(depi))
                if it >= args.warmup:
                    sts.append(st)
            r["fused_ms_total"] = statistics.median(x_["ms_total"] for x_ in sts)
            r["fused_ms_score"] = statistics.median(x_["ms_score"] for x_ in sts)
            r["fused_ms_score_all"] = [x_["ms_score"] for x_ in sts]
        with step_limit(300, "gdca_double_mutants_dev K=%d" % K):
            gen = torch.Generator(device="cuda").manual_seed(K)
            ri = torch.randint(0, N, (L_LIST,), device="cuda", generator=gen)
            rj = (ri + torch.randint(1, N, (L_LIST,), device="cuda", generator=gen)) % N
            rec = torch.stack([torch.randint(0, K, (L_LIST,), device="cuda", generator=gen), ri, torch.randint(1, q + 1, (L_LIST,), device="cuda", generator=gen),
                               rj, torch.randint(1, q + 1, (L_LIST,), device="cuda", generator=gen)], dim=1).to(torch.int32).contiguous()
            dout = torch.empty(L_LIST, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ms = timed(lambda: ctx.double_mutants_dev(ptr(dmJ), ptr(dPi), N, q, ptr(dX), K, ptr(rec), L_LIST, ptr(dout)), args.warmup, args.repeats)
            r["list_1e6_ms"] = statistics.median(ms)
            r["list_1e6_ms_all"] = ms
            r["list_1e6_minus_single_scan_ms"] = r["list_1e6_ms"] - r["single_scan_ms"]
            del rec, dout
        pairs = N * (N - 1) // 2
        r["mutants_ms_scaled"] = res["mutants_one_pair_ms"] * pairs * K

        # ---- floors.  HBM: the off-diagonal blocks of the lower triangle once per sequence chunk, the symbols, dE in, 20 N^2 K bytes out,
        # at k_fn20's fraction of the peak.  VALU: K N (N - 1) / 2 q^2 evaluations of OPS_PER_EVALUATION f64 operations at the add rate.
        chunks = -(-K // CHUNK)
        r["hbm_bytes"] = chunks * 8.0 * s * s * pairs + float(N) * K + 8.0 * q * N * K + 20.0 * N * N * K
        r["hbm_ms_at_fn_rate"] = [r["hbm_bytes"] / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]
        r["evaluations"] = float(K) * pairs * q * q
        r["valu_ms"] = r["evaluations"] * OPS_PER_EVALUATION / (CUS * GHZ * 1e9 * F64_LANES_PER_CLK) * 1e3
        # (a chunk with fewer than 256 sequences still occupies whole waves of 64 lanes)
        lanes = (K // CHUNK) * CHUNK + -(-(K % CHUNK) // 64) * 64
        r["valu_ms_whole_waves"] = r["valu_ms"] * lanes / K
        r["floor_ms"] = max(min(r["hbm_ms_at_fn_rate"]), r["valu_ms"])
        r["binding_floor"] = "valu" if r["valu_ms"] >= min(r["hbm_ms_at_fn_rate"]) else "hbm"
        r["floor_fraction_map_kernel"] = r["floor_ms"] / r["map_kernel_ms"]
        r["floor_fraction_maps_stage"] = r["floor_ms"] / r["maps_stage_ms"]

        # ---- route (b), torch on the same GPU, ONE sequence given the library's dE: blocks gathered, broadcast-add, amin / argmin / norm
        if K == KS[0]:
            with step_limit(300, "torch formulation"):
                ctx.mutation_scan_dev(ptr(dmJ), ptr(dPi), N, q, ptr(dX), 1, gd._lib.MUT_DELTA, ptr(dD))
                torch.cuda.synchronize()
                dE0 = dD[:N * q].view(N, q)
                holder = {}

                def torch_maps():
                    full = torch.tril(mJ) + torch.tril(mJ, -1).t()
                    Bp = torch.zeros((N, q, N, q), dtype=torch.float64, device="cuda")
                    Bp[:, :s, :, :s] = full.view(N, s, N, s)
                    a = x.long() - 1
                    ii = torch.arange(N, device="cuda")
                    Bac = Bp[ii, a]                                       # [i, j, c]
                    Bba = Bp[:, :, ii, a]                                 # [i, b, j]
                    Baa = Bac[:, ii, a]                                   # [i, j]
                    eps = (Bp - Bac[:, None, :, :]) - (Bba[:, :, :, None] - Baa[:, None, :, None])
                    ddE = (dE0[:, :, None, None] + dE0[None, None, :, :]) + eps
                    nb = torch.arange(q, device="cuda")[None, :] != a[:, None]
                    ddE = torch.where(nb[:, :, None, None] & nb[None, None, :, :], ddE, torch.full_like(ddE, float("inf")))
                    flat = ddE.permute(0, 2, 3, 1).reshape(N, N, q * q)   # code = b + q c
                    holder["Emin"], holder["code"] = flat.min(dim=2)
                    holder["epi"] = (eps * eps).sum(dim=(1, 3)).sqrt()

                ms = timed(torch_maps, 1, args.torch_repeats)
                res["torch_one_sequence_ms"] = statistics.median(ms)
                res["torch_one_sequence_ms_all"] = ms
                res["torch_note"] = "one sequence, dE given; the per-K figures are this time SCALED by K"
                ctx.double_mutant_scan_dev(ptr(dmJ), ptr(dPi), N, q, ptr(dX), 1, ptr(dEmin), ptr(dcode), ptr(depi))
                torch.cuda.synchronize()
                off = torch.triu(torch.ones((N, N), dtype=torch.bool, device="cuda"), 1)  # (i < j: the library's orientation)
                lib = dEmin[:N * N].view(N, N).t()                        # [i, j]
                res["torch_vs_map_emin_equal"] = bool(torch.equal(lib[off], holder["Emin"][off]))
                res["torch_vs_map_epi_max_rel"] = float(((depi[:N * N].view(N, N).t() - holder["epi"]).abs()[off] / holder["epi"][off]).max())
                holder.clear()
        r["torch_ms_scaled"] = res["torch_one_sequence_ms"] * K
        r["speedup_vs_mutants"] = r["mutants_ms_scaled"] / r["maps_stage_ms"]
        r["speedup_vs_torch"] = r["torch_ms_scaled"] / r["maps_stage_ms"]
        res["K"][str(K)] = r
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


if __name__ == "__main__":
    main()
