#!/usr/bin/env python3
"""Generate tests/golden/derived_coding2coding_{start,end,join}.jsonl and the same three at --codongapopen -11
--codongapextend -3 --frameshift -13 (derived_coding2coding_codonalt_*): BSDP's derived models of coding2coding (start terminal,
end terminal, join of the match state 2) run by the REFERENCE ITSELF, `oracle/_ref/refdump --cmd golden --derived`, on whole
rectangles.  Runs only where the reference binaries are built; tools/make_golden.py and its sets are left alone.

Inputs are homologous coding pairs with planted events (a one- or two-base frameshift or a whole codon, put into the query or
into the target), as tests/codon_cases.py makes them, plus rectangles with a side of one or two bases and rectangles around the
height of one strip of the derived kernels (64 lanes x 3 rows).  A pool of candidates goes through the reference once per set;
what is written is a selection of at most 40 records, chosen -- and then asserted, the script refuses to write otherwise -- on
the reference's own operation lists:
  * join sets: all nine pairs (query length mod 3, target length mod 3); at least four records each with a query-side
    frameshift, a target-side frameshift, a codon insert and a codon delete;
  * every set: sides of 1 and 2 on each axis; one rectangle one row taller than a strip and one a row shorter;
  * terminal sets: at least four records that begin (end terminal) or end (start terminal) with a frameshift or a gap;
  * rectangles at most 210 x 60, at least three quarters of them at most 49 x 49.
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
ALT_FLAGS = ["--codongapopen", "-11", "--codongapextend", "-3", "--frameshift", "-13"]
# role -> (src state, dst state, start scope, end scope): C4_DerivedModel_create on match state 2 (heuristic.c:242-330)
ROLES = {"start": (0, 2, 0, 4), "end": (2, 1, 4, 0), "join": (2, 2, 4, 4)}
ROWS_PER_LANE = 3                                                   # tools/gen_kernel_tus.py: DERIVED_R["coding2coding"]
STRIP = 64 * ROWS_PER_LANE                                          # query rows (0 ... Q) one strip holds
MAX_RECORDS, MAX_Q, MAX_T, SMALL = 40, 210, 60, 49


def window(rng, ncod, events):
    """A homologous coding pair of ncod codons with the events of cc.EVENT_SHAPE planted at codon boundaries."""
    qc, tc = cc._homologous(rng, [rng.choice(cc.AA) for _ in range(ncod)])
    for kind in events:
        side = qc if kind[0] == "q" else tc
        at = rng.randrange(len(side) + 1)
        side.insert(at, cc._dna(rng, {"1": 1, "2": 2, "c": 3}[kind[1]]))
    return "".join(qc), "".join(tc)


def candidates(rng):
    out = []
    kinds = sorted(cc.EVENT_SHAPE)
    for k in range(240):                                            # BSDP-sized: up to 16 codons, up to two events
        ev = [rng.choice(kinds) for _ in range(rng.choice((0, 1, 1, 1, 2, 2)))]
        q, t = window(rng, rng.randint(1, 14), ev)
        q, t = q[:SMALL], t[:SMALL]
        out.append((q, t))
    for ql, tl in ((1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (2, 3), (3, 2), (1, 7), (7, 1), (2, 8), (8, 2), (1, 12),
                   (12, 2), (2, 30), (31, 1)):                      # a side of one or two bases
        q, t = window(rng, max(ql, tl) // 3 + 1, [])
        out.append((q[:ql], t[:tl]))
    for ql in (STRIP - 2, STRIP - 1, STRIP, STRIP + 1, STRIP - 2, STRIP):      # Q + 1 rows = a strip - 1, a strip, + 1, + 2
        ncod = rng.randint(12, 18)
        q, t = window(rng, ncod, [rng.choice(kinds)])
        filler = "".join(rng.choice(cc.CODONS[rng.choice(cc.AA)]) for _ in range(70))[:ql - len(q)]
        at = 3 * rng.randint(2, ncod - 2)
        q = q[:at] + filler + q[at:]                                # the homologous codons on either side of a long insert
        assert len(q) == ql
        out.append((q, t[:MAX_T]))
    return [("cd%03d" % k, q, t) for k, (q, t) in enumerate(out) if q and t]


def run_reference(cases, role, flags):
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as f:
        for c in cases:
            f.write("%s\t%s\t%s\n" % c)
        path = f.name
    cmd = [REFDUMP, "--cmd", "golden", "--model", "coding2coding", "--input", path, "-D", "32",
           "--derived", "%d,%d,%d,%d" % ROLES[role]] + list(flags)
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout.decode()
    os.unlink(path)
    recs = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert len(recs) == len(cases), (role, len(recs), len(cases))
    for r, c in zip(recs, cases):
        assert r["id"] == c[0]
        r["query"], r["target"], r["dpmemory"] = c[1], c[2], 32
    return recs


def features(model, rec):
    """What the reference's path of this record shows, read off the derived table's transitions."""
    f = {"q%d" % (len(rec["query"]) % 3) + "t%d" % (len(rec["target"]) % 3)}
    if "path_score" not in rec or not rec["ops"]:
        return f
    trs = [model.c.transitions[tr] for tr, _ in rec["ops"]]
    for t in trs:
        name = t.name.decode()
        if name.startswith("frameshift open"):
            f.add("qshift" if t.advance_query else "tshift")
        if name in ("insert", "match to insert"):
            f.add("insert")
        if name in ("delete", "match to delete"):
            f.add("delete")
    if trs[0].name.decode() != "match":
        f.add("begins_off_match")
    if trs[-1].name.decode() != "match":
        f.add("ends_off_match")
    return f


def needs(role):
    n = [(lambda r, f: len(r["query"]) == 1, 1), (lambda r, f: len(r["query"]) == 2, 1),
         (lambda r, f: len(r["target"]) == 1, 1), (lambda r, f: len(r["target"]) == 2, 1),
         (lambda r, f: len(r["query"]) + 1 == STRIP + 1, 1), (lambda r, f: len(r["query"]) + 1 == STRIP - 1, 1)]
    if role == "join":
        n += [(lambda r, f, k="q%dt%d" % (a, b): k in f, 1) for a in range(3) for b in range(3)]
        n += [(lambda r, f, k=k: k in f, 4) for k in ("qshift", "tshift", "insert", "delete")]
    else:
        key = "ends_off_match" if role == "start" else "begins_off_match"
        n += [(lambda r, f: key in f, 4)]
    return n


def select(recs, feats, role, rng):
    chosen = []
    for pred, count in needs(role):
        have = sum(1 for k in chosen if pred(recs[k], feats[k]))
        for k in sorted(range(len(recs)), key=lambda k: len(recs[k]["query"]) * len(recs[k]["target"])):
            if have >= count:
                break
            if k not in chosen and "path_score" in recs[k] and pred(recs[k], feats[k]):
                chosen.append(k)
                have += 1
    rest = [k for k in range(len(recs)) if k not in chosen and len(recs[k]["query"]) <= SMALL]
    rng.shuffle(rest)
    chosen += rest[:MAX_RECORDS - len(chosen)]
    return sorted(chosen)


def check(recs, feats, role):
    assert 0 < len(recs) <= MAX_RECORDS, len(recs)
    assert all(len(r["query"]) <= MAX_Q and len(r["target"]) <= MAX_T for r in recs)
    small = sum(1 for r in recs if len(r["query"]) <= SMALL and len(r["target"]) <= SMALL)
    assert 4 * small >= 3 * len(recs), (small, len(recs))
    for n, (pred, count) in enumerate(needs(role)):
        have = sum(1 for r, f in zip(recs, feats) if pred(r, f))
        assert have >= count, "set %s: requirement %d holds for %d records, %d asked" % (role, n, have, count)


def main():
    if not os.path.exists(REFDUMP):
        sys.exit("oracle/_ref/refdump is not built")
    for tag, flags in (("", []), ("_codonalt", ALT_FLAGS)):
        params = apply_flags(ex.default_params(), flags)
        cases = candidates(random.Random("codon derived" + tag))
        for role, spec in ROLES.items():
            model = ex.Model.derived("coding2coding", *spec, params=params)
            recs = run_reference(cases, role, flags)
            for r in recs:                                          # the builder's table replays the reference's ids
                if "path_score" in r:
                    score, dq, dt, _ = cc.replay(model, r)
                    assert (score, dq, dt) == (r["path_score"], r["region"][2], r["region"][3]), r["id"]
            feats = [features(model, r) for r in recs]
            keep = select(recs, feats, role, random.Random("select" + tag + role))
            recs, feats = [recs[k] for k in keep], [feats[k] for k in keep]
            check(recs, feats, role)
            name = "derived_coding2coding%s_%s" % (tag, role)
            with open(os.path.join(OUT, name + ".jsonl"), "w") as f:
                for r in recs:
                    f.write(json.dumps(r, separators=(",", ":")) + "\n")
            print(name, len(recs), "records,", sum(1 for r in recs if "path_score" in r), "with a path")


if __name__ == "__main__":
    main()
