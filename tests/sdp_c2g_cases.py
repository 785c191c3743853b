"""coding2genome through SDP (the boundary flavour at a query advance of up to 3): the reference-made record sets under
tests/golden/sdp_coding2genome*.jsonl (tools/make_coding2genome_sdp_golden.py), what each was selected to hold -- read off the
reference's own operation lists, here and in the generator alike -- and a seeded fuzz.  Data and table walks only.

The CPU oracle reads the query position of a split-codon calc as an amino acid, so it judges exactly the records whose
alignments hold neither `phase1post ... to (END)` (transition 2) nor `phase2post ... to (END)` (transition 3): oracle_judges().
Everywhere else the checker is the reference's record."""
import random

import exonerate_amd as ex
import coding2genome_cases as cg
from exonerate_amd import _abi
from golden_util import apply_flags, load_set

ALT_FLAGS = ["--frameshift", "-9", "--codongapopen", "-9", "--codongapextend", "-2"]
# set -> parameter flags of the model
SDP_SETS = {"sdp_coding2genome": [], "sdp_coding2genome_altparams": ALT_FLAGS, "sdp_coding2genome_drop": [], "sdp_coding2genome_edges": []}
ADV = (1, 1)                            # refdump grows DNA HSPs from word hits
MAX_RECORDS, MAX_Q = 40, 210
SPLIT_POST = (2, 3)                     # the transitions whose calc the oracle cannot judge for a DNA query
KEYS = ("score", "region", "ops", "vulgar")
_cases = {}


def sdp_case(name):
    """(model, the set's parameters, its records), loaded once."""
    if name not in _cases:
        recs = load_set(name)
        model = ex.Model("coding2genome", params=apply_flags(ex.default_params(), SDP_SETS[name]))
        _cases[name] = (model, recs[0]["params"], recs[1:])
    return _cases[name]


def expected(r):
    return [{"score": a["path_score"], "region": a["region"], "ops": a["ops"], "vulgar": a["vulgar"]} for a in r["alignments"]]


def ids_of(rec):
    return {tr for a in rec["alignments"] for tr, _ in a["ops"]}


def oracle_judges(rec):
    return not (ids_of(rec) & set(SPLIT_POST))


def strips(rec):
    return (len(rec["query"]) + 1 + 63) // 64


def intron_phases(model, aln):
    """The phases of the introns of one alignment, in path order."""
    return [p for p, _, _ in cg.introns_of(model, aln["ops"], aln["region"])]


# ---- strip edges ---------------------------------------------------------------------------------------------------
# The forward pass of the boundary flavour lays its strips from the query's end: a strip's first row is e = Q - 64 k + 1.
EDGE_K = (1, 2)
SPLIT_OFFSETS = tuple(range(-4, 4))
EXIT_OFFSETS = (-1, 0, 1)
EDGE_FEATURES = [("split", p, k, o) for k in EDGE_K for p in (1, 2) for o in SPLIT_OFFSETS] + \
                [("exit0", k, o) for k in EDGE_K for o in EXIT_OFFSETS] + \
                [(kind, k) for k in EDGE_K for kind in ("frameshift", "gap")]


def edge_row(qlen, k):
    return qlen - 64 * k + 1


def edge_features(model, rec):
    """What the reference's paths of a record put on the rows around the strip edges: ("split", phase, k, offset) the first query
    row of a pre-intron split codon at e + offset; ("exit0", k, offset) the 3' splice transition of a phase-0 intron on row
    e + offset; ("frameshift", k) / ("gap", k) one query-side frameshift or codon-gap operation leaving a row below e and
    landing on e or beyond."""
    m, out = model.c, set()
    qlen = len(rec["query"])
    for a in rec["alignments"]:
        i = a["region"][0]
        for tr, length in a["ops"]:
            d = m.transitions[tr]
            name = d.name.decode()
            for _ in range(length):
                for k in EDGE_K:
                    e = edge_row(qlen, k)
                    if e < 1:
                        continue
                    if name.startswith("(START) to phase") and (i - e) in SPLIT_OFFSETS:
                        out.add(("split", int(name[len("(START) to phase")]), k, i - e))
                    if d.label == _abi.LABEL_3SS and name.startswith("intron 0:0") and (i - e) in EXIT_OFFSETS:
                        out.add(("exit0", k, i - e))
                    if d.advance_query and i < e <= i + d.advance_query:
                        if "frameshift" in name:
                            out.add(("frameshift", k))
                        elif "insert" in name:
                            out.add(("gap", k))
                i += d.advance_query
    return out


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------
def word_hits(q, t, w):
    """Every shared word of the pair in target-scan order, as [query position, target position]."""
    words = {}
    for i in range(len(q) - w + 1):
        words.setdefault(q[i:i + w], []).append(i)
    return [(i, j) for j in range(len(t) - w + 1) for i in words.get(t[j:j + w], ())]


def fuzz_pairs(seed, n):
    """Gene pairs for the oracle: homologous coding sequences with events on either axis and introns of PHASE 0 only (a split
    codon's calc is not the oracle's to judge), queries of one to four strips."""
    rng = random.Random("c2g sdp fuzz %d" % seed)
    out = []
    while len(out) < n:
        n_aa = rng.choice((rng.randint(14, 20), rng.randint(22, 41), rng.randint(44, 62), rng.randint(66, 80)))
        n_in = rng.choice((0, 1, 1, 2))
        at = sorted(rng.sample(range(5, n_aa - 5), n_in))
        if any(b - a < 8 for a, b in zip(at, at[1:])):
            continue
        events = [(rng.choice(("q1", "q2", "qc", "q4", "t1", "t2", "tc", "t4")), rng.randrange(4, n_aa - 4)) for _ in range(rng.choice((0, 1, 1, 2)))]
        q, t = cg.gene_pair(rng, n_aa, introns=[(c, 0, rng.randint(30, 90)) for c in at], events=events, flank_q=rng.randrange(3),
                            sub=rng.choice((0.03, 0.1)))
        q += cg.dna(rng, rng.randrange(3))
        if word_hits(q, t, 10):
            out.append((q, t))
    return out
