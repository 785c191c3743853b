#!/usr/bin/env python3
"""coding2genome on one MI355X: one batch of `--pairs` pairs of a CDS of `--qlen` bases against a genomic window of `--tlen`
bases that holds the gene with three introns (phases 0, 1 and 2), through ResidentBatch: warmed up, device-synchronised
(c4gpu_batch_run returns after its read-back).  Prints the first-pass (FIND_SCORE over the whole rectangles) cells/s and the whole
Optimal_find_path step, with the kernel time of one step per pass.  With --reference (where oracle/_ref/exonerate exists) the
same input goes through `exonerate --model coding2genome --exhaustive yes` on one core for `--ref-pairs` of the pairs, and the
cells/s of both are printed side by side.  The numbers of one run are kept in profiles/coding2genome.md.

    python tools/bench_coding2genome.py [--pairs 256] [--qlen 600] [--tlen 20000] [--steps 5] [--reference] [--json out.json]
"""
import argparse, json, os, random, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import exonerate_amd as ex

AA = "ARNDCQEGHILKMFPSTWYV"
_NCBI = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODONS = {}
for _i, _a in enumerate("TCAG"):
    for _j, _b in enumerate("TCAG"):
        for _k, _c in enumerate("TCAG"):
            CODONS.setdefault(_NCBI[_i * 16 + _j * 4 + _k], []).append(_a + _b + _c)
REF_EXONERATE = os.path.join(ROOT, "oracle", "_ref", "exonerate")


def make_pairs(n, qlen, tlen, seed=20261020):
    """A CDS of qlen bases and, somewhere in a random window of tlen bases, its gene: 5 % amino-acid substitutions with synonymous
    codons drawn afresh and three GT ... AG introns of 200 to 2 000 bases, one in each phase."""
    rng = random.Random(seed)
    rnd = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    pairs = []
    for _ in range(n):
        pep = [rng.choice(AA) for _ in range(qlen // 3)]
        qc = [rng.choice(CODONS[a]) for a in pep]
        tc = [rng.choice(CODONS[rng.choice(AA) if rng.random() < 0.05 else a]) for a in pep]
        cuts = sorted(rng.sample(range(10, len(pep) - 10, 12), 3))
        for ph, at in enumerate(cuts):
            for k in range(at - 2, at + 3):
                tc[k] = qc[k]
            body = "GTAAGT" + "".join(rng.choice("ACT") for _ in range(rng.randint(200, 2000) - 18)) + "TTTCTTTTTCAG"
            tc[at] = tc[at][:ph] + body + tc[at][ph:]
        gene = "".join(tc)
        lead = rng.randint(0, tlen - len(gene))
        q = "".join(qc)
        pairs.append((q + rnd(qlen - len(q)), rnd(lead) + gene + rnd(tlen - len(gene) - lead)))
    return pairs


def timed(batch, what, steps, min_seconds):
    """ms per step over at least `steps` steps and `min_seconds` in total"""
    batch.run(what, 32)                                     # warm-up
    done, t0 = 0, time.perf_counter()
    while done < steps or time.perf_counter() - t0 < min_seconds:
        batch.run(what, 32)
        done += 1
    return (time.perf_counter() - t0) * 1e3 / done, done


def reference_seconds(pairs):
    """Wall time of the reference binary on one core over `pairs`, one query against its own window per run."""
    total = 0.0
    with tempfile.TemporaryDirectory() as d:
        for k, (q, t) in enumerate(pairs):
            qf, tf = os.path.join(d, "q.fa"), os.path.join(d, "t.fa")
            with open(qf, "w") as f:
                f.write(">q%d\n%s\n" % (k, q))
            with open(tf, "w") as f:
                f.write(">t%d\n%s\n" % (k, t))
            t0 = time.perf_counter()
            subprocess.run(["taskset", "-c", "0", REF_EXONERATE, "--model", "coding2genome", "--exhaustive", "yes", "--showalignment", "no",
                            "--showvulgar", "yes", qf, tf], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
            total += time.perf_counter() - t0
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--qlen", type=int, default=600)
    ap.add_argument("--tlen", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-pairs", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pairs = make_pairs(a.pairs, a.qlen, a.tlen)
    cells = sum((len(q) + 1) * (len(t) + 1) for q, t in pairs)
    eng = ex.Engine(0)
    model = ex.Model("coding2genome")
    batch = ex.ResidentBatch(eng, model, pairs)
    res = {"pairs": a.pairs, "qlen": a.qlen, "tlen": a.tlen, "first_pass_cells": cells, "device": eng.device_info()["name"]}
    res["score_ms"] = [timed(batch, 0, a.steps, 0.5)[0] for _ in range(2)]
    res["path_ms"] = [timed(batch, 2, a.steps, 0.5)[0] for _ in range(2)]
    res["first_pass_cells_per_s"] = cells / (min(res["score_ms"]) * 1e-3)
    res["find_path_cells_per_s"] = cells / (min(res["path_ms"]) * 1e-3)
    modes = ((0, "score"), (2, "region"), (3, "checkpoint"), (1, "path"))
    for mode, _ in modes:
        batch.kernel_stats(mode, reset=True)
    batch.run(2, 32)
    res["kernel_ms_of_one_find_path"] = {name: batch.kernel_stats(mode)["ms"] for mode, name in modes}
    n = min(64, a.pairs)
    introns = [sum(model.c.transitions[o[0]].label == ex._abi.LABEL_5SS for o in batch.alignment(i).ops) for i in range(n)]
    res["mean_introns_per_alignment"] = sum(introns) / n
    batch.close()
    eng.close()
    print("coding2genome  first pass %8.2f ms  %.3g cells/s   find_path step %8.2f ms  %.3g cells/s   kernels %s   introns per alignment %.2f" % (
        min(res["score_ms"]), res["first_pass_cells_per_s"], min(res["path_ms"]), res["find_path_cells_per_s"],
        {k: round(v, 2) for k, v in res["kernel_ms_of_one_find_path"].items()}, res["mean_introns_per_alignment"]))
    if a.reference and os.path.exists(REF_EXONERATE):
        sub = pairs[:a.ref_pairs]
        secs = reference_seconds(sub)
        # the binary aligns the four strand combinations of a translated pair: four rectangles per pair
        ref_cells = 4 * sum((len(q) + 1) * (len(t) + 1) for q, t in sub)
        res["reference_seconds"], res["reference_pairs"] = secs, len(sub)
        res["reference_cells_per_s"] = ref_cells / secs
        print("reference      %d pairs on one core, four strand combinations each: %.2f s, %.3g cells/s (whole run: find_path included)" % (
            len(sub), secs, res["reference_cells_per_s"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
