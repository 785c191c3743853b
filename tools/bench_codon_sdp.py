#!/usr/bin/env python3
"""coding2coding's SDP on the device, measured (GPU): the library call and the drop-in.

Part 1, the library: the pairs of tests/test_gpu_sdp_codon.py's strip batch (queries of one to five strips, codon HSPs) plus
--pairs homologous coding pairs of up to --qmax bases through Engine.sdp; c4gpu_sdp_stats gives the kernel time of the two
passes and of the walks (HIP events), staging and host time.  The first call is a warm-up (code object load, arena).

Part 2, the drop-in: 64 ORFs of 300-900 nt (eight families of eight diverged copies: tools/bench_codon_seed.py's input) against
each other as heuristic `exonerate-gpu -m coding2coding` (--gappedextension yes, the default), under three settings:
    reference   oracle/_ref/exonerate-compiled, the unmodified reference
    unset       C4GPU_CODON_SDP unset: SDP is the reference's, call for call (the behaviour before the switch existed)
    set         C4GPU_CODON_SDP=1: SDP through c4gpu_sdp_batch
and `set` once more with C4GPU_CODON_SEED=1 C4GPU_SEED_FUSED=1.  Per run: wall time (median of --rounds, min - max), the SDP
seam's own line, and whether the output equals the reference's.  The timing method is tools/bench_codon_seed.py's (wall clock
around the whole process, C4GPU_WAIT=1).  Markdown on stdout."""
import argparse
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GPU_EXE = os.path.join(ROOT, "integration", "_build", "exonerate-gpu")
CPU_EXE = os.path.join(ROOT, "oracle", "_ref", "exonerate-compiled")


def library_part(n_pairs, qmax, rounds):
    import exonerate_amd as ex
    import sdp_codon_cases as sc
    from test_gpu_sdp_codon import _strip_batch
    model, pairs, hsps = _strip_batch()
    rng = random.Random(20261020)
    while len(pairs) < 9 + n_pairs:
        q, t = sc.fuzz_pair(rng, qmax)
        h = sc._codon_hsps(model.params, q, t)
        if h:
            pairs.append((q, t)); hsps.append(h)
    eng = ex.Engine(0)
    eng.sdp(model, pairs, hsps, 3, 3, 50, 40, 4)
    rows = []
    for _ in range(rounds):
        ex.Engine.sdp_stats(reset=True)
        t0 = time.perf_counter()
        got = eng.sdp(model, pairs, hsps, 3, 3, 50, 40, 4)
        wall = (time.perf_counter() - t0) * 1e3
        s = ex.Engine.sdp_stats(reset=True)
        assert all(g is not None for g in got)
        rows.append((wall, s))
    eng.close()
    print("## Engine.sdp: %d pairs (queries of %d-%d bases, %d HSPs), dropoff 50, %d calls after a warm-up\n" %
          (len(pairs), min(len(q) for q, _ in pairs), max(len(q) for q, _ in pairs), sum(len(h) for h in hsps), rounds))
    print("| call | wall ms | passes ms | walks ms | staging ms | host ms | jobs | reruns | unserved |")
    print("|---|---|---|---|---|---|---|---|---|")
    for k, (wall, s) in enumerate(rows):
        print("| %d | %.2f | %.3f | %.3f | %.2f | %.2f | %d | %d | %d |" % (k, wall, s["pass_ms"], s["walk_ms"], s["stage_ms"], s["host_ms"],
                                                                       s["jobs"], s["reruns"], s["unserved"]))
    print()
    sys.stdout.flush()


def dropin_part(rounds, families):
    from bench_codon_seed import orfs
    seqs = orfs(families, 8, 20261020)
    settings = [("reference", CPU_EXE, None), ("unset", GPU_EXE, {}), ("set", GPU_EXE, {"C4GPU_CODON_SDP": "1"}),
                ("set + codon seed, fused", GPU_EXE, {"C4GPU_CODON_SDP": "1", "C4GPU_CODON_SEED": "1", "C4GPU_SEED_FUSED": "1"})]
    print("## exonerate-gpu -m coding2coding (heuristic): %d ORFs of %d-%d nt against each other; wall: median of %d runs (min - max)\n" %
          (len(seqs), min(len(s) for _, s in seqs), max(len(s) for _, s in seqs), rounds))
    print("| setting | wall s | sdp seam | output |")
    print("|---|---|---|---|")
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "orfs.fa")
        with open(fa, "w") as f:
            f.write("".join(">%s\n%s\n" % s for s in seqs))
        args = ["-m", "coding2coding", "--showalignment", "no", "--showvulgar", "yes", "-V", "0", fa, fa]
        ref_out = None
        for name, exe, env in settings:
            walls, err, out = [], "", b""
            for _ in range(rounds):
                t0 = time.perf_counter()
                r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200,
                                   env=dict(os.environ, C4GPU_VERBOSE="1", C4GPU_WAIT="1", **(env or {})))
                walls.append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr.decode()[-1500:]
                out, err = r.stdout, r.stderr.decode()
            if ref_out is None:
                ref_out = out
            m = re.search(r"c4gpu sdp: (\d+ pairs in \d+ flush\(es\): \d+ served from device batches \(\d+ alignments\); batches \d+ ms, replay \d+ ms)", err)
            print("| %s | %.2f (%.2f - %.2f) | %s | %s, %d vulgar lines |" %
                  (name, statistics.median(walls), min(walls), max(walls), m.group(1) if m else "-",
                   "identical" if out == ref_out else "DIFFERS", out.count(b"vulgar:")))
            sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--families", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=247)
    ap.add_argument("--qmax", type=int, default=900)
    ap.add_argument("--skip-dropin", action="store_true")
    a = ap.parse_args()
    library_part(a.pairs, a.qmax, a.rounds)
    if not a.skip_dropin and os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE):
        dropin_part(a.rounds, a.families)


if __name__ == "__main__":
    main()
