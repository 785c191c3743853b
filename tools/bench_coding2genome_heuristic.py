#!/usr/bin/env python3
"""Time the heuristic (BSDP) seam of the drop-in on coding2genome (C4GPU_CODING2GENOME_BSDP=1), written as markdown to stdout
(profiles/coding2genome_heuristic.md).  Wall time of a BSDP-mode run (--gappedextension no) of N CDS queries against N genomic
windows, every query against every window: the drop-in with the switch, the drop-in without it (the reference's route inside the
same binary) and the unmodified reference binary, one after the other, REPS times each (median and range); outputs compared byte
for byte; the seam's own breakdown (dry runs / device / refinement / replay ms, candidates, spans, served calls) from its report
line."""
import os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coding2genome_derived_cases as cd                            # noqa: E402
from codon_derived_cases import GPU_EXE, CPU_EXE                    # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 6
out = sys.argv[2] if len(sys.argv) > 2 else "/tmp/c2g_heur"
REPS = 3
SWITCH = {"C4GPU_CODING2GENOME_BSDP": "1"}
SEEDS = (4242, 11, 12, 13, 14, 15, 16, 17)     # (draws on which the reference itself runs through)
os.makedirs(out, exist_ok=True)
# the genes of the drop-in tests (exons of 28 to 36 codons, introns of every phase, one window on the minus strand), n / 3 draws
qs, ts = [], []
for draw in range((n + 2) // 3):
    dq, dt = cd.cli_inputs(seed=SEEDS[draw])
    qs += [("%s_%d" % (name, draw), seq) for name, seq in dq]
    ts += [("%s_%d" % (name, draw), seq) for name, seq in dt]
for path, recs in ((out + "/q.fa", qs), (out + "/t.fa", ts)):
    with open(path, "w") as f:
        for name, s in recs:
            f.write(">%s\n%s\n" % (name, s))


def run(exe, extra, env=None):
    e = dict(os.environ, C4GPU_VERBOSE="1")
    e.update(env or {})
    args = ["-m", "coding2genome", "--gappedextension", "no", "--showalignment", "no", "--showvulgar", "yes", "-V", "0"] + extra
    t0 = time.perf_counter()
    r = subprocess.run([exe] + args + [out + "/q.fa", out + "/t.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    dt = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    return r.stdout.decode(), dt, r.stderr.decode()


def spread(xs):
    return "%.2f (%.2f ... %.2f)" % (statistics.median(xs), min(xs), max(xs))


run(GPU_EXE, ["-S", "no"], SWITCH)                                   # warm-up (HIP module load)
print("# Heuristic (BSDP) coding2genome runs of the drop-in: %d CDS x %d genomic windows, all against all, four strand pairs\n" % (n, n))
print("Wall seconds, median (range) of %d runs, one after the other on the same machine.\n" % REPS)
print("| flags | reference binary (1 core) | exonerate-gpu, switch off (the reference's route) | exonerate-gpu, C4GPU_CODING2GENOME_BSDP=1 | alignments | candidates (spans) | sub-DP calls answered by device batches | seam: dry runs / device / refinement / replay ms |")
print("|---|---|---|---|---|---|---|---|")
for extra in (["-S", "no"], [], ["--refine", "region"]):
    t_ref, t_off, t_on = [], [], []
    for rep in range(REPS):
        ref, dt, _ = run(CPU_EXE, extra)
        t_ref.append(dt)
        off, dt, _ = run(GPU_EXE, extra)
        t_off.append(dt)
        on, dt, err = run(GPU_EXE, extra, SWITCH)
        t_on.append(dt)
        assert on == ref and off == ref, "outputs differ for %r" % (extra,)
    s = cd.served(err)
    ms = re.search(r"dry runs (\d+) ms, device (\d+) ms, refinement (\d+) ms, replay (\d+) ms", err)
    cand = re.search(r"(\d+) candidate sub-DPs \((\d+) spans\)", err)
    print("| `%s` | %s | %s | %s | %d | %s | %s | %s |" % (" ".join(extra) or "(default)", spread(t_ref), spread(t_off), spread(t_on),
          ref.count("vulgar:"), ("%s (%s)" % cand.groups()) if cand else "?",
          ("%d of %d" % (s[0] + s[2], s[1] + s[3])) if s else "not collected", " / ".join(ms.groups()) if ms else "?"))
print("\nAll outputs byte-identical to the reference's.\n")
