#!/usr/bin/env python3
"""Generate tests/golden/sdp_coding2coding{,_drop,_altparams}.jsonl: SDP (sdp.c:743, the loop of GAM_Result_SDP_create) of the
coding2coding model run by the REFERENCE ITSELF, `oracle/_ref/refdump --cmd sdp --model coding2coding --dnawordlen 10`: the
seeded, bidirectional flavour (use_boundary 0) from the HSPs of the pair's DNA word hits (advances 1/1; SDP takes an HSP only
as a seed point).  Runs only where the reference binaries are built; tools/make_golden.py and its sets are left alone.

Inputs are homologous coding pairs with planted events: one, two, four or five bases (a frameshift) or one to three codons (a
codon gap), put into the query or into the target, between flanks of random bases.  A pool of candidates goes through the
reference once per set; what is written is a selection of at most 40 records, chosen -- and then asserted, the script refuses
to write otherwise -- on the reference's own operation lists:
  * sdp_coding2coding (default --extensionthreshold) and sdp_coding2coding_altparams (--frameshift -9 --codongapopen -9
    --codongapextend -2), together: every transition id of the model; queries of one, two and at least three strips of the
    device passes (64 rows each, Q + 1 >= 129 rows for three); all three residues of Q mod 3;
  * sdp_coding2coding_drop (--extensionthreshold 5 --suboptmax 4 --suboptthreshold 30): at least 10 pairs with two or more
    alignments.
"""
import json, os, random, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exonerate_amd as ex                                          # noqa: E402
import codon_cases as cc                                            # noqa: E402
from golden_util import apply_flags                                 # noqa: E402

REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
OUT = os.path.join(ROOT, "tests", "golden")
ALT_FLAGS = ["--frameshift", "-9", "--codongapopen", "-9", "--codongapextend", "-2"]
SUB = ["--suboptmax", "4", "--suboptthreshold", "40"]
SETS = {"sdp_coding2coding": SUB,
        "sdp_coding2coding_drop": ["--extensionthreshold", "5", "--suboptmax", "4", "--suboptthreshold", "30"],
        "sdp_coding2coding_altparams": ALT_FLAGS + SUB}
WORDLEN, MAX_RECORDS, MAX_Q = 10, 40, 210
EVENTS = {"q1": 1, "q2": 2, "q4": 4, "q5": 5, "qc": 3, "qcc": 6, "qccc": 9,
          "t1": 1, "t2": 2, "t4": 4, "t5": 5, "tc": 3, "tcc": 6, "tccc": 9}


def coding_pair(rng, ncod, events):
    """A homologous coding pair of ncod codons: the target keeps nine codons in ten as they are (DNA words of 10 are shared),
    the events of EVENTS planted at codon boundaries at least five codons apart, flanks of 0-20 random bases."""
    qc = [rng.choice(cc.CODONS[rng.choice(cc.AA)]) for _ in range(ncod)]
    tc = [c if rng.random() < 0.9 else rng.choice(cc.CODONS[rng.choice(cc.AA)]) for c in qc]
    slots = list(range(5, ncod - 4, 5))
    rng.shuffle(slots)
    for kind, at in sorted(zip(events, slots), key=lambda e: -e[1]):
        (qc if kind[0] == "q" else tc).insert(at, cc._dna(rng, EVENTS[kind]))
    return (cc._dna(rng, rng.randint(0, 20)) + "".join(qc) + cc._dna(rng, rng.randint(0, 20)),
            cc._dna(rng, rng.randint(0, 20)) + "".join(tc) + cc._dna(rng, rng.randint(0, 20)))


def word_hits(q, t, w):
    """Every shared word of the pair in target-scan order (what the seeder's scan reports)."""
    words = {}
    for i in range(len(q) - w + 1):
        words.setdefault(q[i:i + w], []).append(i)
    return ["%d:%d" % (i, j) for j in range(len(t) - w + 1) for i in words.get(t[j:j + w], ())]


def candidates(rng):
    out = []
    kinds = sorted(EVENTS)
    while len(out) < 260:
        ncod = rng.choice((rng.randint(12, 19), rng.randint(22, 40), rng.randint(44, 66)))
        ev = [rng.choice(kinds) for _ in range(rng.choice((0, 1, 1, 2, 2, 3)))]
        q, t = coding_pair(rng, ncod, ev)
        q = q[:MAX_Q]
        seeds = word_hits(q, t, WORDLEN)
        if seeds:
            out.append(("c2c%03d" % len(out), q, t, ",".join(seeds)))
    return out


def run_reference(cases, flags):
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as f:
        for c in cases:
            f.write("%s\t%s\t%s\t%s\n" % c)
        path = f.name
    cmd = [REFDUMP, "--cmd", "sdp", "--model", "coding2coding", "--input", path, "--dnawordlen", str(WORDLEN)] + list(flags)
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout.decode()
    os.unlink(path)
    lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    params, recs = lines[0]["params"], lines[1:]
    assert len(recs) == len(cases), (len(recs), len(cases))
    assert params["use_boundary"] == 0 and params["singlepass"] == 1, params
    for r, c in zip(recs, cases):
        assert r["id"] == c[0]
        r["query"], r["target"] = c[1], c[2]
    return params, recs


def strips(rec):
    return (len(rec["query"]) + 1 + 63) // 64


def ids_of(rec):
    return {tr for a in rec["alignments"] for tr, _ in a["ops"]}


def select(recs, wanted, rng):
    """Records that bring a wanted (key, value) nobody chosen so far shows, the smallest first, then a random fill."""
    chosen, have = [], set()
    order = sorted(range(len(recs)), key=lambda k: len(recs[k]["query"]) * len(recs[k]["target"]))
    for need in wanted:
        if need in have:
            continue
        for k in order:
            if recs[k]["alignments"] and need in features(recs[k]):
                if k not in chosen:
                    chosen.append(k)
                have |= features(recs[k])
                break
    rest = [k for k in range(len(recs)) if k not in chosen and recs[k]["alignments"]]
    rng.shuffle(rest)
    chosen += rest[:MAX_RECORDS - len(chosen)]
    return sorted(chosen)


def features(rec):
    return {("id", i) for i in ids_of(rec)} | {("strips", min(3, strips(rec))), ("qmod", len(rec["query"]) % 3)}


def main():
    if not os.path.exists(REFDUMP):
        sys.exit("oracle/_ref/refdump is not built")
    n_tr = ex.Model("coding2coding").c.n_transitions
    wanted = [("id", i) for i in range(n_tr)] + [("strips", s) for s in (1, 2, 3)] + [("qmod", m) for m in range(3)]
    shown = set()
    written = {}
    for name, flags in SETS.items():
        model = ex.Model("coding2coding", params=apply_flags(ex.default_params(), ALT_FLAGS if name.endswith("_altparams") else []))
        cases = candidates(random.Random("codon sdp " + name))
        params, recs = run_reference(cases, flags)
        for r in recs:                                              # the builder's table replays the reference's ids
            for a in r["alignments"]:
                score, dq, dt, _ = cc.replay(model, dict(r, region=a["region"], ops=a["ops"]))
                assert (score, dq, dt) == (a["path_score"], a["region"][2], a["region"][3]), r["id"]
        rng = random.Random("select " + name)
        if name.endswith("_drop"):
            multi = [k for k in range(len(recs)) if len(recs[k]["alignments"]) >= 2]
            rest = [k for k in range(len(recs)) if k not in multi and recs[k]["alignments"]]
            rng.shuffle(multi); rng.shuffle(rest)
            keep = sorted(multi[:24] + rest[:MAX_RECORDS - min(24, len(multi))])
            recs = [recs[k] for k in keep]
            assert sum(1 for r in recs if len(r["alignments"]) >= 2) >= 10
            assert all(a["ops"] for r in recs for a in r["alignments"])
        else:
            recs = [recs[k] for k in select(recs, [w for w in wanted if w not in shown] + wanted, rng)]
            for r in recs:
                shown |= features(r)
        assert 0 < len(recs) <= MAX_RECORDS and all(len(r["query"]) <= MAX_Q for r in recs)
        written[name] = [{"params": params}] + recs
        print(name, len(recs), "records,", sum(len(r["alignments"]) for r in recs), "alignments,",
              sum(1 for r in recs if len(r["alignments"]) >= 2), "pairs with several")
    missing = [w for w in wanted if w not in shown]
    assert not missing, "the default and altparams sets together do not show %r" % (missing,)
    for name, lines in written.items():
        with open(os.path.join(OUT, name + ".jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r, separators=(",", ":")) + "\n")


if __name__ == "__main__":
    main()
