#!/usr/bin/env python3
"""Generate tests/golden/sdp_coding2genome{,_altparams,_drop,_edges}.jsonl: SDP (sdp.c:743, the loop of GAM_Result_SDP_create)
of the coding2genome model run by the REFERENCE ITSELF, `oracle/_ref/refdump --cmd sdp --model coding2genome --dnawordlen 10`:
the boundary flavour (use_boundary 1, three target spans) from the HSPs of the pair's DNA word hits (advances 1/1; SDP takes an
HSP only as a seed point).  Runs only where the reference binaries are built.

A pool of candidates goes through the reference once per set; what is written is a selection of at most 40 records with queries
of at most 210 bases, chosen -- and then asserted, the script refuses to write otherwise -- on the reference's own operation
lists (tests/sdp_c2g_cases.py holds the readers, shared with tests/test_sdp_coding2genome_sets.py):
  * sdp_coding2genome (default) and sdp_coding2genome_altparams (--frameshift -9 --codongapopen -9 --codongapextend -2),
    together: every transition id of the model; queries of one, two and at least three strips of the device passes; all three
    residues of Q mod 3; at least three alignments per intron phase; an alignment with two introns;
  * sdp_coding2genome_drop (--extensionthreshold 5 --suboptmax 4 --suboptthreshold 30): at least 10 pairs with two or more
    alignments;
  * sdp_coding2genome_edges (default): pairs built so that the reference's own path puts a chosen event on a chosen row around a
    forward strip's first row e = Q - 64 k + 1, k = 1 and 2: every feature of sdp_c2g_cases.EDGE_FEATURES.  A candidate whose
    path puts its event elsewhere is dropped; rec["edge"] lists what the record was built for and shows.
Every set holds at least 10 records without a split-codon exit (transitions 2 and 3): the ones the CPU oracle can judge.
"""
import json, os, random, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exonerate_amd as ex                                          # noqa: E402
import coding2genome_cases as cg                                    # noqa: E402
import sdp_c2g_cases as sc                                          # noqa: E402
from golden_util import apply_flags                                 # noqa: E402

REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
OUT = os.path.join(ROOT, "tests", "golden")
SUB = ["--suboptmax", "4", "--suboptthreshold", "40"]
SETS = {"sdp_coding2genome": SUB,
        "sdp_coding2genome_altparams": sc.ALT_FLAGS + SUB,
        "sdp_coding2genome_drop": ["--extensionthreshold", "5", "--suboptmax", "4", "--suboptthreshold", "30"],
        "sdp_coding2genome_edges": SUB}
WORDLEN, MAX_RECORDS, MAX_Q = 10, sc.MAX_RECORDS, sc.MAX_Q
EVENT_BASES = (1, 2, 3, 4, 5, 6, 9)


def random_pair(rng):
    """A CDS of 14-66 codons and its gene: nine codons in ten kept, 0-2 planted events of EVENT_BASES bases on either axis, 0-3
    introns GT...AG of 30-90 bases at random target positions (any phase; the two codons either side kept), flanks."""
    ncod = rng.choice((rng.randint(14, 19), rng.randint(22, 40), rng.randint(44, 66)))
    qc = [rng.choice(cg.CODONS[rng.choice(cg.AA)]) for _ in range(ncod)]
    tc = [c if rng.random() < 0.9 else rng.choice(cg.CODONS[rng.choice(cg.AA)]) for c in qc]
    for at in sorted(rng.sample(range(3, ncod - 3), rng.choice((0, 1, 1, 2, 3))), reverse=True):
        ph = rng.randrange(3)
        for k in range(at - 2, at + 3):
            if len(tc[k]) == 3:
                tc[k] = qc[k]
        tc[at] = tc[at][:ph] + cg.intron(rng, rng.randint(30, 90)) + tc[at][ph:]
    slots = list(range(5, ncod - 4, 5))
    rng.shuffle(slots)
    for at in sorted(slots[:rng.choice((0, 1, 1, 2))], reverse=True):
        (qc if rng.random() < 0.5 else tc).insert(at, cg.dna(rng, rng.choice(EVENT_BASES)))
    q = cg.dna(rng, rng.randint(0, 20)) + "".join(qc) + cg.dna(rng, rng.randint(0, 20))
    return q[:MAX_Q], cg.dna(rng, rng.randint(0, 20)) + "".join(tc) + cg.dna(rng, rng.randint(0, 20))


def candidates(rng, n=300):
    out = []
    while len(out) < n:
        q, t = random_pair(rng)
        seeds = sc.word_hits(q, t, WORDLEN)
        if seeds:
            out.append(("c2g%03d" % len(out), q, t, ",".join("%d:%d" % s for s in seeds)))
    return out


# ---- pairs for the strip edges ----------------------------------------------------------------------------------------
def k_of(feature):
    return feature[2] if feature[0] == "split" else feature[1]


def edge_pair(rng, feats):
    """A pair whose path should show `feats` (one per k, k = 2 first): (query, target) or None when the rows do not come out as
    whole codons for any tail of 0-2 bases."""
    feats = sorted(feats, key=lambda f: -k_of(f))
    ks = [k_of(f) for f in feats]
    n_aa = rng.randint(58 if 2 in ks else 30, 66)
    flank = rng.randrange(3)
    wants = []                                                      # (row offset from e of the event's first row, query extras)
    for f in feats:
        if f[0] == "split":
            wants.append((f[3], 0))
        elif f[0] == "exit0":
            wants.append((f[2], 0))
        elif f[0] == "frameshift":
            extra = rng.choice((1, 2))
            wants.append((-rng.randint(1, extra), extra))
        else:
            wants.append((-rng.randint(1, 3), 3))
    extras = sum(x for _, x in wants)
    for tail in rng.sample(range(3), 3):
        qlen = flank + 3 * n_aa + extras + tail
        if qlen > MAX_Q:
            continue
        before, cis = 0, []
        for (off, x), k in zip(wants, ks):
            row = sc.edge_row(qlen, k) + off
            if row - flank - before < 15 or (row - flank - before) % 3:
                break
            cis.append((row - flank - before) // 3)
            before += x
        else:
            if all(6 <= c <= n_aa - 6 for c in cis) and all(b - a >= 8 for a, b in zip(cis, cis[1:])):
                introns, events = [], []
                for f, c, (_, x) in zip(feats, cis, wants):
                    if f[0] == "split":
                        introns.append((c, f[1], rng.randint(30, 90)))
                    elif f[0] == "exit0":
                        introns.append((c, 0, rng.randint(30, 90)))
                    elif f[0] == "frameshift":
                        events.append(("q%d" % x, c))
                    else:
                        events.append(("qc", c))
                q, t = cg.gene_pair(rng, n_aa, introns=introns, events=events, flank_q=flank, sub=0.03, keep=4)
                q += cg.dna(rng, tail)
                assert len(q) == qlen
                return q, t
    return None


def edge_candidates(rng):
    """Singles of every feature (several draws) and doubles (one feature at k = 2, one at k = 1) of every combination whose rows
    come out; each with the features it was built for."""
    out, built = [], []
    k1 = [f for f in sc.EDGE_FEATURES if k_of(f) == 1]
    k2 = [f for f in sc.EDGE_FEATURES if f not in k1]
    plans = [[f] for f in sc.EDGE_FEATURES for _ in range(4)] + [[a, b] for a in k2 for b in k1 for _ in range(2)]
    for feats in plans:
        pair = edge_pair(rng, feats)
        if pair and sc.word_hits(pair[0], pair[1], WORDLEN):
            q, t = pair
            out.append(("c2e%04d" % len(out), q, t, ",".join("%d:%d" % s for s in sc.word_hits(q, t, WORDLEN))))
            built.append(feats)
    return out, built


def run_reference(cases, flags):
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as f:
        for c in cases:
            f.write("%s\t%s\t%s\t%s\n" % c)
        path = f.name
    cmd = [REFDUMP, "--cmd", "sdp", "--model", "coding2genome", "--input", path, "--dnawordlen", str(WORDLEN)] + list(flags)
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout.decode()
    os.unlink(path)
    lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    params, recs = lines[0]["params"], lines[1:]
    assert len(recs) == len(cases), (len(recs), len(cases))
    assert params["use_boundary"] == 1 and params["singlepass"] == 1 and params["n_spans"] == 3, params
    for r, c in zip(recs, cases):
        assert r["id"] == c[0]
        r["query"], r["target"] = c[1], c[2]
    return params, recs


def features(model, rec):
    out = {("id", i) for i in sc.ids_of(rec)} | {("strips", min(3, sc.strips(rec))), ("qmod", len(rec["query"]) % 3)}
    for a in rec["alignments"]:
        ph = sc.intron_phases(model, a)
        out |= {("phase", p) for p in ph}
        if len(ph) >= 2:
            out.add(("two introns",))
    return out


def cover(recs, feats_of, needs, rng, fill_from=None, cap=MAX_RECORDS):
    """Greedy: while a need is open, the record that closes most open needs (the smallest among equals); then a random fill of
    records from fill_from up to `cap`.  needs: {feature: count}."""
    chosen, open_ = [], dict(needs)
    size = lambda k: len(recs[k]["query"]) * len(recs[k]["target"])
    while any(v > 0 for v in open_.values()):
        best = max((k for k in range(len(recs)) if k not in chosen and recs[k]["alignments"]),
                   key=lambda k: (sum(1 for f in feats_of[k] if open_.get(f, 0) > 0), -size(k)), default=None)
        if best is None or not any(open_.get(f, 0) > 0 for f in feats_of[best]):
            break
        chosen.append(best)
        for f in feats_of[best]:
            if open_.get(f, 0) > 0:
                open_[f] -= 1
    rest = [k for k in (fill_from if fill_from is not None else range(len(recs))) if k not in chosen and recs[k]["alignments"]]
    rng.shuffle(rest)
    chosen += rest[:max(0, cap - len(chosen))]
    return sorted(chosen), {f: v for f, v in open_.items() if v > 0}


def check_paths(model, recs):
    for r in recs:                                                  # the builder's table replays the reference's ids
        for a in r["alignments"]:
            _, dq, dt, _ = cg.replay(model, r, ops=a["ops"], region=a["region"])
            assert (dq, dt) == (a["region"][2], a["region"][3]), r["id"]


def main():
    if not os.path.exists(REFDUMP):
        sys.exit("oracle/_ref/refdump is not built")
    n_tr = ex.Model("coding2genome").c.n_transitions
    needs = dict([(("id", i), 1) for i in range(n_tr)] + [(("strips", s), 1) for s in (1, 2, 3)] + [(("qmod", m), 1) for m in range(3)] +
                 [(("phase", p), 3) for p in range(3)] + [(("two introns",), 1)])
    written, still = {}, dict(needs)
    for name, flags in SETS.items():
        model = ex.Model("coding2genome", params=apply_flags(ex.default_params(), sc.SDP_SETS[name]))
        rng = random.Random("select " + name)
        if name.endswith("_edges"):
            cases, built = edge_candidates(random.Random("c2g sdp " + name))
            params, recs = run_reference(cases, flags)
            check_paths(model, recs)
            shown = [sc.edge_features(model, r) for r in recs]
            ok = [k for k in range(len(recs)) if set(built[k]) <= shown[k]]          # the reference chose otherwise: dropped
            recs, built = [recs[k] for k in ok], [built[k] for k in ok]
            for r, b in zip(recs, built):
                r["edge"] = [list(f) for f in b]
            free = [k for k in range(len(recs)) if sc.oracle_judges(recs[k])]
            split_needs = {f: 1 for f in sc.EDGE_FEATURES if f[0] == "split"}
            free_needs = {f: 1 for f in sc.EDGE_FEATURES if f[0] != "split"}
            keep_a, miss_a = cover(recs, [set(b) for b in built], split_needs, rng, fill_from=[])
            sub = [recs[k] for k in free]
            keep_b, miss_b = cover(sub, [set(built[k]) for k in free], free_needs, rng, cap=MAX_RECORDS - len(keep_a))
            assert not miss_a and not miss_b, "the edges pool does not show %r" % (sorted(miss_a) + sorted(miss_b),)
            recs = [recs[k] for k in sorted(set(keep_a) | {free[k] for k in keep_b})]
            have = set().union(*[{tuple(f) for f in r["edge"]} for r in recs])
            assert have == set(sc.EDGE_FEATURES), sorted(set(sc.EDGE_FEATURES) - have)
            for r in recs:
                assert {tuple(f) for f in r["edge"]} <= sc.edge_features(model, r), r["id"]
        else:
            cases = candidates(random.Random("c2g sdp " + name))
            params, recs = run_reference(cases, flags)
            check_paths(model, recs)
            feats = [features(model, r) for r in recs]
            if name.endswith("_drop"):
                multi = [k for k in range(len(recs)) if len(recs[k]["alignments"]) >= 2]
                free = [k for k in range(len(recs)) if k not in multi and recs[k]["alignments"] and sc.oracle_judges(recs[k])]
                rest = [k for k in range(len(recs)) if k not in multi and k not in free and recs[k]["alignments"]]
                rng.shuffle(multi); rng.shuffle(free); rng.shuffle(rest)
                keep = multi[:20] + free[:12]
                keep = sorted(keep + rest[:MAX_RECORDS - len(keep)])
                recs = [recs[k] for k in keep]
                assert sum(1 for r in recs if len(r["alignments"]) >= 2) >= 10
            else:
                keep, _ = cover(recs, feats, still, rng)
                recs = [recs[k] for k in keep]
                for r in recs:
                    for f in features(model, r):
                        if still.get(f, 0) > 0:
                            still[f] -= 1
        assert 0 < len(recs) <= MAX_RECORDS and all(len(r["query"]) <= MAX_Q for r in recs)
        assert all(a["ops"] for r in recs for a in r["alignments"])
        assert sum(1 for r in recs if r["alignments"] and sc.oracle_judges(r)) >= 10, name
        written[name] = [{"params": params}] + recs
        print(name, len(recs), "records,", sum(len(r["alignments"]) for r in recs), "alignments,",
              sum(1 for r in recs if len(r["alignments"]) >= 2), "pairs with several,",
              sum(1 for r in recs if r["alignments"] and sc.oracle_judges(r)), "for the oracle")
    missing = {f: v for f, v in still.items() if v > 0}
    assert not missing, "the default and altparams sets together do not show %r" % (missing,)
    for name, lines in written.items():
        with open(os.path.join(OUT, name + ".jsonl"), "w") as f:
            for r in lines:
                f.write(json.dumps(r, separators=(",", ":")) + "\n")


if __name__ == "__main__":
    main()
