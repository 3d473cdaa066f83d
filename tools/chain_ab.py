#!/usr/bin/env python3
"""One process, one library (GDCA_LIB selects another build), one config: the figures of tools/sample_bench.py, tools/temper_bench.py
and tools/walk_bench.py that the shared chain body (csrc/gdca_chain.h) could move, for an A/B of two libraries in alternating
processes -- the tools' shapes, sequences, seeds, proposal counts and timing function (imported from them), WITHOUT their old-route,
floor, rule-length-launch and bisection parts, the betas 0.5 and 2 and the walk at max_steps = 32, and with 6 timed calls after 1 at
K = 8192 where the tools take 10 after 2.  Prints one line "RESULT <json>".

    GDCA_LIB=<parent's libgdca.so> python tools/chain_ab.py C;  python tools/chain_ab.py C      (B likewise; alternate, >= 4 pairs)
    python tools/chain_ab.py B rejected    only K = 1, 256 at beta = 0 and 1e9 (the rejected proposal's figure)"""
import json
import statistics
import sys
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mutation_bench import CONFIGS, KS, step_limit, timed  # noqa: E402
import temper_bench  # noqa: E402

config = sys.argv[1]
import gaussdca.jl_amd as gd  # noqa: E402
from gaussdca.jl_amd import devops  # noqa: E402
from gaussdca.jl_amd.synth import synth_family  # noqa: E402

c = CONFIGS[config]
N, M, q, theta, pc = c["N"], c["M"], 21, c["theta"], 0.8
n = N * (q - 1)
TK, TR = temper_bench.K, temper_bench.R
G = TK * TR
stream = torch.cuda.current_stream()
with step_limit(60, "contexts"):
    ctx = gd.Context(0, stream=stream.cuda_stream)
    torch.cuda.synchronize()
Zo = synth_family(N, M, q, c["seed"])
KMAX = max(KS)
X = np.random.default_rng(c["seed"]).integers(1, q, size=(KMAX, N)).astype(np.int8)
with step_limit(60, "upload"):
    dZ = torch.from_numpy(Zo).cuda()
    dX = torch.from_numpy(X).cuda()
    dD = torch.empty(KMAX * N * q, dtype=torch.float64, device="cuda")
    dXs = torch.empty((KMAX, N), dtype=torch.int8, device="cuda")
    dXo = torch.empty((G, N), dtype=torch.int8, device="cuda")
    dacc = torch.empty(KMAX, dtype=torch.int32, device="cuda")
    dsw = torch.empty(TK * (TR - 1), dtype=torch.int32, device="cuda")
    dso = torch.empty(G, dtype=torch.int32, device="cuda")
    dsteps = torch.empty(KMAX, dtype=torch.int32, device="cuda")
    dsum = torch.empty(KMAX, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
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


def chains(K, beta, T):
    ctx.sample_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), K, None, 0, beta, 1, 0, T - 1, 1, 1, dXs.data_ptr(), dacc.data_ptr())


def walk(K, T):
    ctx.greedy_walk_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), K, None, 0, 0.0, T, dXout_ptr, dsteps.data_ptr(), dsum.data_ptr())


dXout_ptr = dXs.data_ptr()
REJ = sys.argv[2:] == ["rejected"]
res = dict(config=config, lib=os.environ.get("GDCA_LIB", "this"))
for K in (KS[:2] if REJ else KS):
    T = 4096 if K <= 256 else 1024
    W, R = (2, 10) if K <= 256 else (1, 6)
    with step_limit(120, "scan"):
        scan = statistics.median(timed(lambda: ctx.mutation_scan_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), K, gd._lib.MUT_POTENTIAL,
                                                                     dD.data_ptr()), W, R))
    res["K%d_scan_ms" % K] = scan
    for beta in ((0.0, 1e9) if REJ else (1.0, 0.0, 1e9)):
        with step_limit(300, "sample K=%d beta=%g" % (K, beta)):
            ms = statistics.median(timed(lambda: chains(K, beta, T), W, R))
            acc = float(dacc[:K].cpu().numpy().astype(np.int64).sum())
        kern = ms - scan
        if beta == 1.0:
            res["K%d_call_beta1_ms" % K] = ms
        elif beta == 0.0:
            res["K%d_ns_per_accepted_move" % K] = kern * 1e6 / acc
        else:
            res["K%d_ns_per_proposal_beta1e9" % K] = kern * 1e6 / (K * T)
            res["K%d_acceptance_beta1e9" % K] = acc / (K * T)
    if REJ:
        continue
    with step_limit(300, "walk K=%d" % K):
        ms = statistics.median(timed(lambda: walk(K, 4 * N), W, R))
        steps = dsteps[:K].cpu().numpy().astype(np.int64)
    res["K%d_walk4N_ms_per_step" % K] = (ms - scan) / float(steps.max())
if REJ:
    ctx.close()
    print("RESULT " + json.dumps(res, sort_keys=True), flush=True)
    sys.exit(0)
# the tempered call of tools/temper_bench.py: K = 256 chains of R = 8 replicas, swap_every = N, 16 sweeps, a geometric ladder from 1 to 0.3
T = 16 * N
betas = [float(b) for b in np.geomspace(1.0, 0.3, TR)]
Xg = np.random.default_rng(c["seed"]).integers(1, q, size=(G, N)).astype(np.int8)
dXr = torch.from_numpy(Xg).cuda()
dXs2 = torch.empty((G, N), dtype=torch.int8, device="cuda")
dacc2 = torch.empty(G, dtype=torch.int32, device="cuda")
with step_limit(400, "tempered"):
    ms = timed(lambda: ctx.sample_tempered_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dXr.data_ptr(), None, TK, betas, None, 0, 1, 0, N, T - N, N, 1,
                                               dXs2.data_ptr(), dacc2.data_ptr(), dsw.data_ptr(), dXo.data_ptr(), dso.data_ptr()), 2, 10)
res["tempered_call_ms"] = statistics.median(ms)
ctx.close()
print("RESULT " + json.dumps(res, sort_keys=True), flush=True)
