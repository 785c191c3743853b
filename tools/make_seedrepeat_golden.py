#!/usr/bin/env python3
"""tests/golden/hsp_seedrepeat_{dna2dna,protein2protein}.jsonl: what the reference BINARY prints (exonerate -m ungapped
--showsugar yes, built by oracle/Makefile into oracle/_ref/) for small pairs under --seedrepeat 1, 2 and 3 (hspset.c:950-970: a
horizon entry's counter and its diagonal tag), as run_hsp_softmask of tools/make_golden.py records the soft-mask options.  Every
pair records its HSPs [query_start, target_start, length, score] per repeat value.  The inputs: copies of exactly w, w + 1 and
w + 2 identical symbols with mismatching flanks (1, 2 and 3 word hits on one diagonal), single-word copies one query length apart
(two diagonals on one entry: the tag), w + 1 copies one query length apart, a long copy, and a diagonal with a second HSP past the
first one's horizon.  A set is written only if the reference's own outputs show that the option decides: repeat 2 removes at
least 6 HSPs against repeat 1, repeat 3 at least 3 more, and the tag pair keeps nothing at repeat 2."""
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_EXONERATE = os.path.join(ROOT, "oracle", "_ref", "exonerate")
OUT = os.path.join(ROOT, "tests", "golden")
AA = "ARNDCQEGHILKMFPSTWYV"
SETS = {"dna2dna": dict(seedlen=12, dropoff=30, threshold=40, target_advance=1, alphabet="ACGT", qlen=100, types=("dna", "dna"),
                        flags=["--dnahspthreshold", "40"]),
        "protein2protein": dict(seedlen=6, dropoff=20, threshold=20, target_advance=1, alphabet=AA, qlen=60,
                                types=("protein", "protein"), flags=["--proteinhspthreshold", "20", "--proteinwordlimit", "0"])}
REPEATS = (1, 2, 3)


def rand(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def other(rng, c, alphabet):
    return rng.choice([x for x in alphabet if x != c])


def planted(rng, q, spots, alphabet, tlen):
    """A random target with q[p:p + n] at `at` for every (p, n, at), the symbol on either side of a copy unlike the query's own
    neighbour on that diagonal: the copy gives exactly n - w + 1 word hits."""
    t = list(rand(rng, tlen, alphabet))
    for p, n, at in spots:
        t[at:at + n] = q[p:p + n]
        if p > 0 and at > 0:
            t[at - 1] = other(rng, q[p - 1], alphabet)
        if p + n < len(q) and at + n < tlen:
            t[at + n] = other(rng, q[p + n], alphabet)
    return "".join(t)


def cases(match, seed):
    par = SETS[match]
    rng = random.Random(seed)
    a, w, qlen = par["alphabet"], par["seedlen"], par["qlen"]
    out = []
    q = lambda: rand(rng, qlen, a)
    for k in range(3):                                       # exactly w, w + 1, w + 2 symbols: 1, 2, 3 word hits
        for v in "ab":
            x = q()
            out.append(("copy_w%d_%s" % (k, v), x, planted(rng, x, [(20, w + k, 31)], a, 90)))
    x = q()
    out.append(("tag", x, planted(rng, x, [(25, w, 20), (25, w, 20 + qlen)], a, 2 * qlen + 40)))
    x = q()
    out.append(("tag_w1", x, planted(rng, x, [(25, w + 1, 20), (25, w + 1, 20 + qlen)], a, 2 * qlen + 40)))
    x = q()
    out.append(("three_singles", x, planted(rng, x, [(5, w, 10), (30, w, 60), (qlen - w - 3, w, 110)], a, 160)))
    x = q()
    out.append(("long", x, rand(rng, 17, a) + x + rand(rng, 9, a)))
    x = q()                                                  # two HSPs on one diagonal: the middle third replaced by mismatches
    third = qlen // 3
    out.append(("two_on_a_diagonal", x, rand(rng, 11, a) + x[:third] + "".join(other(rng, c, a) for c in x[third:2 * third]) +
                x[2 * third:] + rand(rng, 6, a)))
    return out


def reference_hsps(par, cid, q, t, seed_repeat):
    flags = ["-m", "ungapped", "-Q", par["types"][0], "-T", par["types"][1], "--showsugar", "yes", "--showalignment", "no",
             "--showvulgar", "no", "--score", "1", "-V", "0"] + par["flags"] + ["--seedrepeat", str(seed_repeat)]
    with tempfile.TemporaryDirectory() as d:
        qf, tf = os.path.join(d, "q.fa"), os.path.join(d, "t.fa")
        with open(qf, "w") as f:
            f.write(">%s\n%s\n" % (cid, q))
        with open(tf, "w") as f:
            f.write(">tg_%s\n%s\n" % (cid, t))
        r = subprocess.run([REF_EXONERATE] + flags + [qf, tf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    hsps = []
    for l in r.stdout.decode().split("\n"):
        if not l.startswith("sugar:"):
            continue
        s = l.split()                                        # sugar: qid qstart qend qstrand tid tstart tend tstrand score
        if s[4] == "-" or s[8] == "-":                       # a chance hit on a reverse strand: not part of these records
            continue
        hsps.append([int(s[2]), int(s[6]), int(s[3]) - int(s[2]), int(s[9])])
        assert int(s[7]) - int(s[6]) == hsps[-1][2] * par["target_advance"], l
    return sorted(hsps), flags[:-2]


def run(match):
    par = SETS[match]
    recs, flags = [], None
    for cid, q, t in cases(match, 7300 + len(match)):
        assert len(q) <= (240 if match == "dna2dna" else 80) and len(t) <= 900, (cid, len(q), len(t))
        rec = {"id": cid, "query": q, "target": t, "repeat": {}}
        for r in REPEATS:
            rec["repeat"][str(r)], flags = reference_hsps(par, cid, q, t, r)
        recs.append(rec)
    count = lambda r: sum(len(x["repeat"][str(r)]) for x in recs)
    assert count(1) - count(2) >= 6, (match, "repeat 2 removes only", count(1) - count(2))
    assert count(2) - count(3) >= 3, (match, "repeat 3 removes only", count(2) - count(3), "more")
    for x in recs:
        if x["id"] == "tag":
            assert len(x["repeat"]["1"]) == 2 and x["repeat"]["2"] == [], x
    head = {k: par[k] for k in ("seedlen", "dropoff", "threshold", "target_advance")}
    head.update(match=match, flags=flags, repeats=list(REPEATS))
    name = "hsp_seedrepeat_" + match
    with open(os.path.join(OUT, name + ".jsonl"), "w") as f:
        f.write(json.dumps({"params": head}, separators=(",", ":")) + "\n")
        for x in recs:
            f.write(json.dumps(x, separators=(",", ":")) + "\n")
    print(name, len(recs), "pairs; HSPs at repeat 1, 2, 3:", count(1), count(2), count(3))


if __name__ == "__main__":
    for m in sys.argv[1:] or sorted(SETS):
        run(m)
