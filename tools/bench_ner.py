#!/usr/bin/env python3
"""ner against affine:local on one MI355X: the same seeded DNA pairs through ResidentBatch, in one process and alternating, warmed
up, device-synchronised (c4gpu_batch_run returns after its read-back).  Prints the first-pass (FIND_SCORE over the whole
rectangles) cells/s of both models, the whole Optimal_find_path step of both, and -- where the reference binary is present -- the
reference's one-core time for `--model ner --exhaustive yes --subopt no` on a 16-pair subset, whose vulgar lines must be the
device's.  The numbers of one run are kept in profiles/ner_bench.md / .json.

    python tools/bench_ner.py [--pairs 1024] [--qlen 1000] [--tlen 20000] [--steps 5] [--json out.json]
"""
import argparse, json, os, random, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import exonerate_amd as ex

REF = os.path.join(ROOT, "oracle", "_ref", "exonerate-compiled")


def make_pairs(n, qlen, tlen, seed=20261016):
    """Three conserved blocks (5 % substitutions) with unrelated inserts of different lengths between them, somewhere in a random
    target: alignments that ner joins through NER operations and affine:local through gaps (or not at all)."""
    rng = random.Random(seed)
    rnd = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    sub = lambda s: "".join(rng.choice("ACGT") if rng.random() < 0.05 else c for c in s)
    pairs = []
    for _ in range(n):
        b = [rnd((qlen - 90) // 3) for _ in range(3)]
        q = rnd(20) + b[0] + rnd(30) + b[1] + rnd(12) + b[2]
        q += rnd(qlen - len(q))
        core = sub(b[0]) + rnd(11) + sub(b[1]) + rnd(44) + sub(b[2])
        lead = rng.randint(0, tlen - len(core))
        pairs.append((q, rnd(lead) + core + rnd(tlen - len(core) - lead)))
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
    ap.add_argument("--qlen", type=int, default=1000)
    ap.add_argument("--tlen", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--ref-pairs", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pairs = make_pairs(a.pairs, a.qlen, a.tlen)
    cells = sum((len(q) + 1) * (len(t) + 1) for q, t in pairs)
    eng = ex.Engine(0)
    models = {"ner": ex.Model("ner"), "affine:local": ex.Model("affine:local")}
    batches = {k: ex.ResidentBatch(eng, m, pairs) for k, m in models.items()}
    res = {"pairs": a.pairs, "qlen": a.qlen, "tlen": a.tlen, "first_pass_cells": cells, "device": eng.device_info()["name"]}
    for rnd_ in range(2):                                   # alternating: ner, affine, ner, affine
        for k in ("ner", "affine:local"):
            ms, n = timed(batches[k], 0, a.steps, 0.5)
            res.setdefault(k, {}).setdefault("score_ms", []).append(ms)
            ms, n = timed(batches[k], 2, a.steps, 0.5)
            res[k].setdefault("path_ms", []).append(ms)
    for k in models:
        r = res[k]
        r["score_ms_best"], r["path_ms_best"] = min(r["score_ms"]), min(r["path_ms"])
        r["first_pass_cells_per_s"] = cells / (r["score_ms_best"] * 1e-3)
        r["find_path_cells_per_s"] = cells / (r["path_ms_best"] * 1e-3)
        for mode, name in ((0, "score"), (2, "region"), (3, "checkpoint"), (1, "path")):
            batches[k].kernel_stats(mode, reset=True)
        batches[k].run(2, 32)
        r["kernel_ms_of_one_find_path"] = {name: batches[k].kernel_stats(mode)["ms"]
                                           for mode, name in ((0, "score"), (2, "region"), (3, "checkpoint"), (1, "path"))}
    res["ratio_first_pass"] = res["ner"]["first_pass_cells_per_s"] / res["affine:local"]["first_pass_cells_per_s"]
    res["ratio_find_path"] = res["ner"]["find_path_cells_per_s"] / res["affine:local"]["find_path_cells_per_s"]
    if os.path.exists(REF) and a.ref_pairs > 0:
        n = min(a.ref_pairs, a.pairs)
        mine = [batches["ner"].alignment(i).vulgar("qy%d" % i, "tg%d" % i) for i in range(n)]
        t_ref, same = 0.0, 0
        with tempfile.TemporaryDirectory() as d:
            for i in range(n):
                qf, tf = os.path.join(d, "q.fa"), os.path.join(d, "t.fa")
                open(qf, "w").write(">qy%d\n%s\n" % (i, pairs[i][0]))
                open(tf, "w").write(">tg%d\n%s\n" % (i, pairs[i][1]))
                t0 = time.perf_counter()
                out = subprocess.run([REF, "-m", "ner", "-E", "yes", "-S", "no", "-n", "1", "--revcomp", "no", "--showalignment", "no",
                                      "--showvulgar", "yes", "-V", "0", qf, tf], stdout=subprocess.PIPE, check=True).stdout.decode()
                t_ref += time.perf_counter() - t0
                same += [l for l in out.splitlines() if l.startswith("vulgar:")] == [mine[i]]
        res["reference"] = {"pairs": n, "seconds_one_core": t_ref, "cells_per_s": cells * n / a.pairs / t_ref,
                            "identical_vulgar_lines": same}
    for b in batches.values():
        b.close()
    eng.close()
    for k in models:
        print("%-13s first pass %8.2f ms  %.3g cells/s   find_path step %8.2f ms  %.3g cells/s   kernels %s" % (
            k, res[k]["score_ms_best"], res[k]["first_pass_cells_per_s"], res[k]["path_ms_best"], res[k]["find_path_cells_per_s"],
            {n: round(v, 2) for n, v in res[k]["kernel_ms_of_one_find_path"].items()}))
    print("ner / affine:local: first pass %.3f, find_path step %.3f" % (res["ratio_first_pass"], res["ratio_find_path"]))
    if "reference" in res:
        print("reference, one core: %d pairs in %.1f s (%.3g cells/s), %d of %d vulgar lines identical" % (
            res["reference"]["pairs"], res["reference"]["seconds_one_core"], res["reference"]["cells_per_s"],
            res["reference"]["identical_vulgar_lines"], res["reference"]["pairs"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
