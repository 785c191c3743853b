#!/usr/bin/env python3
"""coding2genome's SDP on the device, measured (GPU): the library call and the drop-in.

Input: --cds CDS of 300-900 bases and, for each, a genomic window of 2-5 kb that holds its gene: 5 % of the residues replaced,
synonymous codons drawn afresh, three GT ... AG introns of 100 to 800 bases, one in each phase (tools/bench_coding2genome.py's
generator at these sizes).

Part 1, the library: every CDS against its own window through Engine.sdp from the DNA HSPs of the pair's word hits (advances
1/1); c4gpu_sdp_stats gives the kernel time of the two passes and of the walks (HIP events), staging and host time.  The first
call is a warm-up (code object load, arena).

Part 2, the drop-in: all CDS against all windows as heuristic `exonerate-gpu -m coding2genome` (--gappedextension yes, the
default), under three settings:
    reference   oracle/_ref/exonerate-compiled, the unmodified reference
    unset       C4GPU_CODING2GENOME_SDP unset: SDP is the reference's, call for call, inside the same binary (the parent's route)
    set         C4GPU_CODING2GENOME_SDP=1: SDP through c4gpu_sdp_batch
Per run: wall time (median of --rounds, min - max), the SDP seam's own line, and whether the output equals the reference's.  The
timing method is tools/bench_codon_sdp.py's (wall clock around the whole process, C4GPU_WAIT=1).  Markdown on stdout."""
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


def genes(n, seed=20261023):
    """[(cds, window)]: the CDS and the window with its gene.  (The seed is one on which the unmodified reference runs to its end: on
    some inputs of this shape, seeds 20261021 and 20261022 among them, it stops with "Initial HSP score [-1] less than zero".)"""
    from bench_coding2genome import AA, CODONS
    rng = random.Random(seed)
    rnd = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    out = []
    for _ in range(n):
        pep = [rng.choice(AA) for _ in range(rng.randint(100, 300))]
        qc = [rng.choice(CODONS[a]) for a in pep]
        tc = [rng.choice(CODONS[rng.choice(AA) if rng.random() < 0.05 else a]) for a in pep]
        cuts = sorted(rng.sample(range(10, len(pep) - 10, 12), 3))
        phases = [0, 1, 2]
        rng.shuffle(phases)
        for ph, at in zip(phases, cuts):
            for k in range(at - 2, at + 3):
                tc[k] = qc[k]
            body = "GTAAGT" + "".join(rng.choice("ACT") for _ in range(rng.randint(100, 800) - 18)) + "TTTCTTTTTCAG"
            tc[at] = tc[at][:ph] + body + tc[at][ph:]
        out.append(("".join(qc), rnd(rng.randint(200, 900)) + "".join(tc) + rnd(rng.randint(200, 900))))
    return out


def library_part(pairs, rounds):
    import exonerate_amd as ex
    import sdp_codon_cases
    model = ex.Model("coding2genome")
    hsps = [sdp_codon_cases._dna_hsps(model.params, q, t) for q, t in pairs]
    eng = ex.Engine(0)
    eng.sdp(model, pairs, hsps, 1, 1, 50, 40, 4)
    rows = []
    for _ in range(rounds):
        ex.Engine.sdp_stats(reset=True)
        t0 = time.perf_counter()
        got = eng.sdp(model, pairs, hsps, 1, 1, 50, 40, 4)
        wall = (time.perf_counter() - t0) * 1e3
        s = ex.Engine.sdp_stats(reset=True)
        assert all(g is not None for g in got)
        rows.append((wall, s))
    eng.close()
    five = ex._abi.LABEL_5SS
    introns = [sum(n for tr, n in a.ops if model.c.transitions[tr].label == five) for g in got for a in g[:1]]
    print("## Engine.sdp: %d pairs (queries of %d-%d bases, targets of %d-%d, %d HSPs), dropoff 50, %d calls after a warm-up\n" %
          (len(pairs), min(len(q) for q, _ in pairs), max(len(q) for q, _ in pairs), min(len(t) for _, t in pairs),
           max(len(t) for _, t in pairs), sum(len(h) for h in hsps), rounds))
    print("| call | wall ms | passes ms | walks ms | staging ms | host ms | jobs | reruns | unserved |")
    print("|---|---|---|---|---|---|---|---|---|")
    for k, (wall, s) in enumerate(rows):
        print("| %d | %.2f | %.3f | %.3f | %.2f | %.2f | %d | %d | %d |" % (k, wall, s["pass_ms"], s["walk_ms"], s["stage_ms"], s["host_ms"],
                                                                       s["jobs"], s["reruns"], s["unserved"]))
    print("\nIntrons in the best alignment of a pair: %.2f on average (three planted).\n" % (sum(introns) / max(1, len(introns))))
    sys.stdout.flush()


def dropin_part(pairs, rounds):
    settings = [("reference", CPU_EXE, None), ("unset", GPU_EXE, {}), ("set", GPU_EXE, {"C4GPU_CODING2GENOME_SDP": "1"})]
    print("## exonerate-gpu -m coding2genome (heuristic): %d CDS of %d-%d nt against %d windows of %d-%d nt; wall: median of %d runs (min - max)\n" %
          (len(pairs), min(len(q) for q, _ in pairs), max(len(q) for q, _ in pairs), len(pairs), min(len(t) for _, t in pairs),
           max(len(t) for _, t in pairs), rounds))
    print("| setting | wall s | sdp seam | output |")
    print("|---|---|---|---|")
    with tempfile.TemporaryDirectory() as tmp:
        qf, tf = os.path.join(tmp, "cds.fa"), os.path.join(tmp, "genes.fa")
        with open(qf, "w") as f:
            f.write("".join(">cds%d\n%s\n" % (k, q) for k, (q, _) in enumerate(pairs)))
        with open(tf, "w") as f:
            f.write("".join(">gene%d\n%s\n" % (k, t) for k, (_, t) in enumerate(pairs)))
        args = ["-m", "coding2genome", "--showalignment", "no", "--showvulgar", "yes", "-V", "0", qf, tf]
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
            print("| %s | %.2f (%.2f - %.2f) | %s | %s, %d vulgar lines, %d with an intron |" %
                  (name, statistics.median(walls), min(walls), max(walls), m.group(1) if m else "-",
                   "identical" if out == ref_out else "DIFFERS", out.count(b"vulgar:"),
                   sum(1 for l in out.decode().splitlines() if l.startswith("vulgar:") and " I " in l)))
            sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cds", type=int, default=64)
    ap.add_argument("--skip-dropin", action="store_true")
    a = ap.parse_args()
    pairs = genes(a.cds)
    library_part(pairs, a.rounds)
    if not a.skip_dropin and os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE):
        dropin_part(pairs, a.rounds)


if __name__ == "__main__":
    main()
