#!/usr/bin/env python3
"""Heuristic runs of the translated models through the drop-in, with and without the opt-in codon seeding (GPU).

64 ORFs of 300-900 nt (eight families of eight diverged copies, so that there is something to find) against each other, as
`exonerate-gpu -m ungapped:trans` and `-m coding2coding`, under three settings:
    off     C4GPU_CODON_SEED unset: the seeding is the reference's, call for call (the behaviour before the switch existed)
    on      C4GPU_CODON_SEED=1: word scan (c4gpu_seed_scan) and HSP extensions (c4gpu_hsp_extend_chains, codon2codon)
    fused   ... and C4GPU_SEED_FUSED=1: one c4gpu_seed_extend call per target
with the unmodified reference (oracle/_ref/exonerate-compiled) alongside.  Per run: wall time (median of --rounds), and the
seams' own milliseconds from their C4GPU_VERBOSE lines.  Every output is compared with the reference's.  Markdown on stdout."""
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
GPU_EXE = os.path.join(ROOT, "integration", "_build", "exonerate-gpu")
CPU_EXE = os.path.join(ROOT, "oracle", "_ref", "exonerate-compiled")
TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
SENSE = [a + b + c for a in "TCAG" for b in "TCAG" for c in "TCAG" if TABLE["TCAG".index(a) * 16 + "TCAG".index(b) * 4 + "TCAG".index(c)] != "*"]


def orfs(n_families, per_family, seed):
    rng = random.Random(seed)
    out = []
    for f in range(n_families):
        base = [rng.choice(SENSE) for _ in range(rng.randint(100, 300))]
        for k in range(per_family):
            copy = [rng.choice(SENSE) if rng.random() < 0.12 else c for c in base]
            lo = rng.randint(0, len(copy) - 100)
            hi = rng.randint(lo + 100, len(copy))
            out.append(("orf%d_%d" % (f, k), "".join(copy[lo:hi])))
    return out


def seam_ms(err):
    """The seams' own numbers: (word scan ms incl. delivery and tables, HSP ms, fused ms)."""
    scan = re.search(r"scans ([\d.]+) ms, delivery ([\d.]+) ms, word tables \(\d+ words, \d+ emissions\) ([\d.]+) ms", err)
    hsp = re.search(r"device batch\(es\) \(([\d.]+) ms", err)
    fused = re.search(r"HSPs kept \(([\d.]+) ms", err)
    return (sum(float(x) for x in scan.groups()) if scan else None, float(hsp.group(1)) if hsp else None,
            float(fused.group(1)) if fused else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--families", type=int, default=8)
    a = ap.parse_args()
    seqs = orfs(a.families, 8, 20261020)
    settings = [("reference", CPU_EXE, None), ("off", GPU_EXE, {}), ("on", GPU_EXE, {"C4GPU_CODON_SEED": "1"}),
                ("fused", GPU_EXE, {"C4GPU_CODON_SEED": "1", "C4GPU_SEED_FUSED": "1"})]
    print("%d ORFs of %d-%d nt against each other; wall: median of %d runs (min - max)\n" %
          (len(seqs), min(len(s) for _, s in seqs), max(len(s) for _, s in seqs), a.rounds))
    print("| model | setting | wall s | word scan ms | HSP seam ms | fused ms | output |")
    print("|---|---|---|---|---|---|---|")
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "orfs.fa")
        with open(fa, "w") as f:
            f.write("".join(">%s\n%s\n" % s for s in seqs))
        for model in ("ungapped:trans", "coding2coding"):
            args = ["-m", model, "--showalignment", "no", "--showvulgar", "yes", "-V", "0", fa, fa]
            ref_out = None
            for name, exe, env in settings:
                walls, err, out = [], "", b""
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200,
                                       env=dict(os.environ, C4GPU_VERBOSE="1", C4GPU_WAIT="1", **(env or {})))
                    walls.append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr.decode()[-1500:]
                    out, err = r.stdout, r.stderr.decode()
                if ref_out is None:
                    ref_out = out
                scan, hsp, fused = seam_ms(err) if env is not None else (None, None, None)
                f = lambda x: "-" if x is None else "%.0f" % x
                print("| %s | %s | %.2f (%.2f - %.2f) | %s | %s | %s | %s, %d vulgar lines |" %
                      (model, name, statistics.median(walls), min(walls), max(walls), f(scan), f(hsp), f(fused),
                       "identical" if out == ref_out else "DIFFERS", out.count(b"vulgar:")))
                sys.stdout.flush()


if __name__ == "__main__":
    main()
