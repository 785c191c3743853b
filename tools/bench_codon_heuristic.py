#!/usr/bin/env python3
"""Time the heuristic (BSDP) seam on coding2coding and the derived codon launches behind it.  Two measurements, each repeated
REPS times (median and range reported), written as markdown to stdout (profiles/codon_heuristic.md):
  1. wall time of the drop-in on a BSDP-mode coding2coding run (--gappedextension no) of N homologous coding pairs, every query
     against every target (N x N comparisons, N = 16: a few hundred), against the same binary with --gpu no and against the
     unmodified reference; outputs compared byte for byte;
  2. jobs per second of one launch of 3 000 rectangles of 1 ... 49 by 1 ... 49 under the derived join model of coding2coding,
     against the affine join launch of tests/test_gpu_parity.py::test_thousands_of_bsdp_sized_jobs_on_derived_models."""
import os, random, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exonerate_amd as ex                                          # noqa: E402
import codon_derived_cases as cd                                    # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
out = sys.argv[2] if len(sys.argv) > 2 else "/tmp/codon_heur"
REPS = 3
os.makedirs(out, exist_ok=True)
qs, ts = cd.coding_pairs(n, seed=20261019)
for path, recs in ((out + "/q.fa", qs), (out + "/t.fa", ts)):
    with open(path, "w") as f:
        for name, s in recs:
            f.write(">%s\n%s\n" % (name, s))


def run(exe, extra, env=None):
    e = dict(os.environ, C4GPU_VERBOSE="1")
    e.update(env or {})
    args = ["-m", "coding2coding", "--gappedextension", "no", "--showalignment", "no", "--showvulgar", "yes", "-V", "0"] + extra
    t0 = time.perf_counter()
    r = subprocess.run([exe] + args + [out + "/q.fa", out + "/t.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    dt = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    return r.stdout.decode(), dt, r.stderr.decode()


def spread(xs):
    return "%.2f (%.2f ... %.2f)" % (statistics.median(xs), min(xs), max(xs))


run(cd.GPU_EXE, ["-S", "no"])                                        # warm-up (HIP module load)
print("# Heuristic (BSDP) coding2coding runs of the drop-in: %d queries x %d targets, all against all, four strand pairs\n" % (n, n))
print("Wall seconds, median (range) of %d runs.\n" % REPS)
print("| flags | reference binary (1 core) | exonerate-gpu | exonerate-gpu --gpu no | alignments | sub-DP calls answered by device batches | seam: dry runs / device / refinement / replay ms |")
print("|---|---|---|---|---|---|---|")
for extra in (["-S", "no"], [], ["--refine", "region"]):
    t_ref, t_gpu, t_no = [], [], []
    for rep in range(REPS):
        ref, dt, _ = run(cd.CPU_EXE, extra)
        t_ref.append(dt)
        gpu, dt, err = run(cd.GPU_EXE, extra)
        t_gpu.append(dt)
        no, dt, _ = run(cd.GPU_EXE, extra + ["--gpu", "no"])
        t_no.append(dt)
        assert gpu == ref and no == ref, "outputs differ for %r" % (extra,)
    s = cd.served(err)
    ms = re.search(r"dry runs (\d+) ms, device (\d+) ms, refinement (\d+) ms, replay (\d+) ms", err)
    print("| `%s` | %s | %s | %s | %d | %s | %s |" % (" ".join(extra) or "(default)", spread(t_ref), spread(t_gpu), spread(t_no),
          ref.count("vulgar:"), ("%d of %d" % (s[0] + s[2], s[1] + s[3])) if s else "not collected",
          " / ".join(ms.groups()) if ms else "?"))
print("\nAll outputs byte-identical to the reference's.\n")

# ---- one launch of 3 000 derived jobs ------------------------------------------------------------------------------------
eng = ex.Engine(0)
print("# One launch of 3 000 BSDP-sized rectangles (1 ... 49 by 1 ... 49) of one pair, FIND_PATH and FIND_SCORE\n")
print("Thousand jobs per second through `Engine.viterbi` (upload, launch, download), median (range) of %d launches after a warm-up.\n" % REPS)
print("| derived model | rows per lane | FIND_PATH kjobs/s | FIND_SCORE kjobs/s |")
print("|---|---|---|---|")
for mt, spec, rows in (("affine:local", (2, 2, 4, 4), 1), ("coding2coding", (2, 2, 4, 4), 3), ("coding2coding", (0, 2, 0, 4), 3),
                       ("coding2coding", (2, 1, 4, 0), 3)):
    rng = random.Random(2024)
    q = "".join(rng.choice("ACGT") for _ in range(1500))
    t = "".join(rng.choice("ACGT") if rng.random() < 0.12 else c for c in q) + "".join(rng.choice("ACGT") for _ in range(300))
    model = ex.Model.derived(mt, *spec)
    jobs = []
    for k in range(3000):
        ql, tl = rng.randint(1, 49), rng.randint(2, 49)
        jobs.append({"pair": 0, "region": (rng.randint(0, len(q) - ql), rng.randint(0, len(t) - tl), ql, tl)})
    rates = {}
    for mode in (ex.MODE_FIND_PATH, ex.MODE_FIND_SCORE):
        eng.viterbi(model, mode, [(q, t)], jobs)
        xs = []
        for rep in range(REPS):
            t0 = time.perf_counter()
            eng.viterbi(model, mode, [(q, t)], jobs)
            xs.append(len(jobs) / (time.perf_counter() - t0) / 1e3)
        rates[mode] = "%.0f (%.0f ... %.0f)" % (statistics.median(xs), min(xs), max(xs))
    print("| %s %r | %d | %s | %s |" % (mt, spec, rows, rates[ex.MODE_FIND_PATH], rates[ex.MODE_FIND_SCORE]))
eng.close()
