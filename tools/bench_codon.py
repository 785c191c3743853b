#!/usr/bin/env python3
"""coding2coding against affine:local on one MI355X: the same seeded coding DNA pairs through ResidentBatch, in one process and
alternating, warmed up, device-synchronised (c4gpu_batch_run returns after its read-back).  Prints the first-pass (FIND_SCORE over
the whole rectangles) cells/s of both models and the whole Optimal_find_path step of both, with the kernel time of one step per
mode.  The numbers of one run are kept in profiles/codon_bench.md / .json.

    python tools/bench_codon.py [--pairs 1024] [--qlen 999] [--tlen 6000] [--steps 5] [--json out.json]
"""
import argparse, json, os, random, sys, time
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


def make_pairs(n, qlen, tlen, seed=20261017):
    """A coding query of qlen bases and, somewhere in a random target of tlen bases, a homologue of it: 8 % amino-acid
    substitutions with synonymous codons drawn afresh, two codon indels and one one-base frameshift."""
    rng = random.Random(seed)
    rnd = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    pairs = []
    for _ in range(n):
        pep = [rng.choice(AA) for _ in range(qlen // 3)]
        q = "".join(rng.choice(CODONS[a]) for a in pep)
        tc = [rng.choice(CODONS[rng.choice(AA) if rng.random() < 0.08 else a]) for a in pep]
        for _x in range(2):
            at = rng.randrange(10, len(tc) - 10)
            tc[at:at] = [rng.choice(CODONS[rng.choice(AA)])]
        tc[rng.randrange(10, len(tc) - 10)] += rng.choice("ACGT")
        core = "".join(tc)
        lead = rng.randint(0, tlen - len(core))
        pairs.append((q + rnd(qlen - len(q)), rnd(lead) + core + rnd(tlen - len(core) - lead)))
    return pairs


def timed(batch, what, steps, min_seconds):
    """ms per step over at least `steps` steps and `min_seconds` in total"""
    batch.run(what, 32)                                     # warm-up
    done, t0 = 0, time.perf_counter()
    while done < steps or time.perf_counter() - t0 < min_seconds:
        batch.run(what, 32)
        done += 1
    return (time.perf_counter() - t0) * 1e3 / done, done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--qlen", type=int, default=999)
    ap.add_argument("--tlen", type=int, default=6000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pairs = make_pairs(a.pairs, a.qlen, a.tlen)
    cells = sum((len(q) + 1) * (len(t) + 1) for q, t in pairs)
    eng = ex.Engine(0)
    order = ("coding2coding", "affine:local")
    models = {k: ex.Model(k) for k in order}
    batches = {k: ex.ResidentBatch(eng, m, pairs) for k, m in models.items()}
    res = {"pairs": a.pairs, "qlen": a.qlen, "tlen": a.tlen, "first_pass_cells": cells, "device": eng.device_info()["name"]}
    for _round in range(2):                                 # alternating: coding2coding, affine, coding2coding, affine
        for k in order:
            ms, n = timed(batches[k], 0, a.steps, 0.5)
            res.setdefault(k, {}).setdefault("score_ms", []).append(ms)
            ms, n = timed(batches[k], 2, a.steps, 0.5)
            res[k].setdefault("path_ms", []).append(ms)
    for k in order:
        r = res[k]
        r["score_ms_best"], r["path_ms_best"] = min(r["score_ms"]), min(r["path_ms"])
        r["first_pass_cells_per_s"] = cells / (r["score_ms_best"] * 1e-3)
        r["find_path_cells_per_s"] = cells / (r["path_ms_best"] * 1e-3)
        for mode, name in ((0, "score"), (2, "region"), (3, "checkpoint"), (1, "path")):
            batches[k].kernel_stats(mode, reset=True)
        batches[k].run(2, 32)
        r["kernel_ms_of_one_find_path"] = {name: batches[k].kernel_stats(mode)["ms"]
                                           for mode, name in ((0, "score"), (2, "region"), (3, "checkpoint"), (1, "path"))}
        r["mean_aligned_query_bases"] = sum(batches[k].alignment(i).region[2] for i in range(min(64, a.pairs))) / min(64, a.pairs)
    res["ratio_first_pass"] = res[order[0]]["first_pass_cells_per_s"] / res[order[1]]["first_pass_cells_per_s"]
    res["ratio_find_path"] = res[order[0]]["find_path_cells_per_s"] / res[order[1]]["find_path_cells_per_s"]
    for b in batches.values():
        b.close()
    eng.close()
    for k in order:
        print("%-13s first pass %8.2f ms  %.3g cells/s   find_path step %8.2f ms  %.3g cells/s   kernels %s   aligned query bases %.0f" % (
            k, res[k]["score_ms_best"], res[k]["first_pass_cells_per_s"], res[k]["path_ms_best"], res[k]["find_path_cells_per_s"],
            {n: round(v, 2) for n, v in res[k]["kernel_ms_of_one_find_path"].items()}, res[k]["mean_aligned_query_bases"]))
    print("coding2coding / affine:local: first pass %.3f, find_path step %.3f" % (res["ratio_first_pass"], res["ratio_find_path"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
