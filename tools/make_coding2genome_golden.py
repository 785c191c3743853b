#!/usr/bin/env python3
"""Generate the coding2genome vectors under tests/golden/ by running the REFERENCE ITSELF: oracle/_ref/refdump (its `golden`
command takes any Model_Type name) and oracle/_ref/exonerate, both built by `make -C oracle ref` where the reference tree is.
The pairs come from the seeded generators of tests/coding2genome_cases.py (no reference code).  Sets (each a few kB):
  coding2genome.jsonl          -D 32; rec["ss"]: the 5' / 3' splice values at the sites the path uses (refdump --withsplice,
                               thinned to those positions), so that tests/test_coding2genome_model.py can add the score up
  coding2genome_D0.jsonl       -D 0 (checkpoints and continuations)
  coding2genome_alt.jsonl      rec["point"] = altparams | tightintron (golden_util.PARAM_VARIANTS)
  coding2genome_subopt.jsonl   the GAM sub-optimal loop (--suboptmax 4 --suboptthreshold 30)
  codon_cli_coding2genome.json stdout of exonerate --model coding2genome --exhaustive yes with --showalignment, vulgar and
                               --showtargetgff: one run per pair, the second with the gene on the target's minus strand
"""
import json, os, random, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coding2genome_cases as cc                                     # noqa: E402
from golden_util import PARAM_VARIANTS                                # noqa: E402

REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
REF_EXONERATE = os.path.join(ROOT, "oracle", "_ref", "exonerate")
OUT = os.path.join(ROOT, "tests", "golden")


def run(cases, dpmemory, extra=()):
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as f:
        for c in cases:
            f.write("%s\t%s\t%s\n" % c)
        path = f.name
    cmd = [REFDUMP, "--cmd", "golden", "--model", "coding2genome", "--input", path, "-D", str(dpmemory)] + list(extra)
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout.decode()
    os.unlink(path)
    recs = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert [r["id"] for r in recs] == [c[0] for c in cases]
    for r, c in zip(recs, cases):
        r["query"], r["target"], r["dpmemory"] = c[1], c[2], dpmemory
        assert r.get("ops"), r["id"]                                  # every record carries a path
    return recs


def thin_splice(model, rec):
    """Keeps of the four splice arrays only the forward values at the first target position of the path's site transitions."""
    ss = {"5": {}, "3": {}}
    j = rec["region"][1]
    for tr, length in rec["ops"]:
        t = model.c.transitions[tr]
        if t.label == cc._abi.LABEL_5SS:
            ss["5"][str(j)] = rec["ss5_forward"][j]
        if t.label == cc._abi.LABEL_3SS:
            ss["3"][str(j)] = rec["ss3_forward"][j]
        j += t.advance_target * length
    for k in ("ss5_forward", "ss3_forward", "ss5_reverse", "ss3_reverse"):
        del rec[k]
    rec["ss"] = ss


def short_cases(rng, tag):
    """Queries of 1 to 5 bases out of an exon, and of 18 and 19 bases whose middle lies on an exon junction."""
    out = []
    for ql in (1, 2, 3, 4, 5, 18, 19):
        q, t = cc.gene_pair(rng, 24, introns=[(12, ql % 3, 30 + ql)], flank_t=4, sub=0.0)
        at = 36 - ql // 2 if ql >= 18 else rng.randrange(0, 30)
        out.append(("%s%02d" % (tag, ql), q[at:at + ql], t))
    return out


def main():
    model = cc.point_model("default")
    rng = random.Random(5353)
    shaped = [dict(n_aa=30, introns=[(15, 0, 40)]), dict(n_aa=32, introns=[(16, 1, 45)], flank_q=1),
              dict(n_aa=32, introns=[(17, 2, 52)], flank_q=2), dict(n_aa=54, introns=[(16, 1, 36), (36, 2, 44)]),
              dict(n_aa=50, introns=[(24, 0, 38)], events=[("q1", 10), ("tc", 38), ("tc", 38)]),
              dict(n_aa=50, introns=[(24, 1, 41)], events=[("t2", 11), ("qc", 37), ("qc", 37)]),
              dict(n_aa=50, introns=[(26, 2, 47)], events=[("q2", 10), ("t1", 39)], flank_q=1),
              dict(n_aa=44, introns=[(22, 0, 36)], events=[("q4", 9), ("t4", 34)])]
    base = [("g%03d" % k, ) + cc.gene_pair(rng, **sp) for k, sp in enumerate(shaped)]
    main_cases = base + short_cases(rng, "gs") + \
        [("gl%d" % ql, ) + cc.query_of_length(rng, ql, introns=[(ql // 3 - 8 - k, k % 3, 40 + 7 * k)], flank_t=4) for k, ql in enumerate((191, 192))]
    recs = run(main_cases, 32, ["--withsplice", "yes"])
    for r in recs:
        thin_splice(model, r)
    write("coding2genome", recs)
    d0 = [("d%03d" % k, ) + cc.gene_pair(rng, **sp) for k, sp in enumerate(shaped[:6])] + \
        [("dl%d" % ql, ) + cc.query_of_length(rng, ql, introns=[(60 + k, (k + 1) % 3, 45 + 5 * k)], flank_t=4) for k, ql in enumerate((383, 384, 385, 386))]
    write("coding2genome_D0", run(d0, 0))
    alt = [("a%03d" % k, ) + cc.gene_pair(rng, **sp) for k, sp in enumerate(shaped[:4])] + \
        [("al%d" % ql, ) + cc.query_of_length(rng, ql, introns=[(40 + k, 2 - k, 50 + 9 * k)], flank_t=4) for k, ql in enumerate((193, 194))] + \
        [("al600", ) + cc.query_of_length(rng, 600, introns=[(64, 1, 120), (130, 2, 44)], flank_t=3)]
    alt_recs = run(alt, 32, PARAM_VARIANTS["altparams"])
    for r in alt_recs:
        r["point"] = "altparams"
    # --minintron 77 --maxintron 78: introns of exactly either length and one base outside either
    tight = [("t%d" % n, ) + cc.gene_pair(rng, 36, introns=[(18, n % 3, n)], flank_t=5, sub=0.0) for n in (76, 77, 78, 79)]
    tight_recs = run(tight, 32, PARAM_VARIANTS["tightintron"])
    for r in tight_recs:
        r["point"] = "tightintron"
    write("coding2genome_alt", alt_recs + tight_recs)
    # the sub-optimal loop: a second, diverged copy of the gene further along the target
    sub = []
    for k, sp in enumerate(shaped[:4]):
        q, t = cc.gene_pair(rng, **sp)
        copy = "".join(rng.choice("ACGT") if rng.random() < 0.05 else c for c in t[10:-10])
        sub.append(("s%03d" % k, q, t + cc.dna(rng, 9 + k) + copy))
    sub_recs = run(sub, 32, cc.SUBOPT_FLAGS)
    for r in sub_recs:
        for a in r.get("subopt", []):
            a.pop("points", None)
    write(cc.SUBOPT_SET, sub_recs)
    run_cli(rng)


def write(name, recs):
    path = os.path.join(OUT, name + ".jsonl")
    with open(path, "w") as f:
        for r in recs:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(name, len(recs), "records,", os.path.getsize(path), "bytes, scores", [r["score"] for r in recs[:8]])


def run_cli(rng):
    pairs = [("cg0", ) + cc.gene_pair(rng, 30, introns=[(14, 1, 38)], flank_q=1, flank_t=6), ("cg1", ) + cc.gene_pair(rng, 36, introns=[(12, 2, 33), (25, 0, 41)], flank_t=6)]
    pairs[1] = (pairs[1][0], pairs[1][1], cc.revcomp(pairs[1][2]))
    out = {"model": "coding2genome", "flags": [], "reports": cc.CLI_REPORTS, "pairs": []}
    for cid, q, t in pairs:
        with tempfile.TemporaryDirectory() as d:
            qf, tf = os.path.join(d, "q.fa"), os.path.join(d, "t.fa")
            with open(qf, "w") as f:
                f.write(">%s cds\n%s\n" % (cid, q))
            with open(tf, "w") as f:
                f.write(">tg_%s\n%s\n" % (cid, t))
            cmd = [REF_EXONERATE, "--model", "coding2genome", "--exhaustive", "yes"] + cc.CLI_REPORTS + [qf, tf]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        lines = [l for l in r.stdout.decode().split("\n") if not l.startswith(("Command line:", "Hostname:", "##date "))]
        recs = []
        for v in [l.split() for l in lines if l.startswith("vulgar:")]:
            # the same alignments as transition ids: refdump on the strands the binary chose
            qs, ts = v[4], v[8]
            rec = run([(cid, cc.revcomp(q) if qs == "-" else q, cc.revcomp(t) if ts == "-" else t)], 32)[0]
            if rec["vulgar"].split()[10:] == v[10:] and rec["path_score"] == int(v[9]):
                recs.append({"qstrand": qs, "tstrand": ts, "score": rec["path_score"], "region": rec["region"], "ops": rec["ops"]})
        assert len(recs) == sum(l.startswith("vulgar:") for l in lines) >= 1, cid
        out["pairs"].append({"id": cid, "qdef": "cds", "tid": "tg_" + cid, "query": q, "target": t, "stdout": lines, "alignments": recs})
    path = os.path.join(OUT, cc.CLI_SET + ".json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(cc.CLI_SET, len(out["pairs"]), "pairs,", os.path.getsize(path), "bytes,", [[a["tstrand"] for a in p["alignments"]] for p in out["pairs"]])


if __name__ == "__main__":
    main()
