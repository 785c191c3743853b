"""Pin the oracle's 3:3 match (oracle/c4_oracle.c, C4GPU_CALC_MATCH_CODON) on the reference: on every recorded set of the
translated models (tests/golden/coding2coding*.jsonl, ungapped_trans*.jsonl, codon_cli_*.json) and, where build() made
oracle/_ref/refdump, on the reference run on the spot over the generated bands of tests/codon_cases.py -- queries of one to five
256-row strips, which no record reaches.  That live check is what licenses tests/test_gpu_codon_oracle.py to hold the device
kernels to the oracle at those sizes.  Integer work and text: every comparison is exact."""
import json
import os
import random
import subprocess
import tempfile

import pytest

import oracle_lib
from golden_util import expected
from codon_cases import (REFDUMP_SETS, SUBOPT_SETS, CLI_SETS, SUBOPT_MAX, POINTS, ALL_POINTS, EDGE_POINTS, BANDS, STRIP, set_model, load_set,
                         load_cli, strand_seqs, edge_pairs, fuzz_pair, band_shows, band_rng, point_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")


@pytest.mark.parametrize("name", sorted(REFDUMP_SETS))
def test_oracle_matches_reference_vectors(lib, name):
    model = set_model(name)
    recs = load_set(name)
    assert recs
    for rec in recs:
        q, t = rec["query"].encode(), rec["target"].encode()
        assert oracle_lib.find_score(model.c, model.params, q, t) == rec["score"], rec["id"]
        got = oracle_lib.find_path(model.c, model.params, q, t, dpmemory=rec["dpmemory"], qid=rec["id"])
        if "path_score" not in rec:
            assert got is None, rec["id"]
            continue
        assert got == expected(rec), rec["id"]


@pytest.mark.parametrize("name", sorted(SUBOPT_SETS))
def test_oracle_suboptimal_loop_matches_reference(lib, name):
    """SubOpt blocking under an advance of 3 (a 3:3 match blocks the three cells of its diagonal): the successive alignments."""
    model = set_model(name)
    rounds = 0
    for rec in load_set(name):
        q, t = rec["query"].encode(), rec["target"].encode()
        got = oracle_lib.find_paths_subopt(model.c, model.params, q, t, rec["dpmemory"], rec["threshold"], SUBOPT_MAX, qid=rec["id"])
        assert [(d["score"], d["region"], d["ops"], d["vulgar"]) for d, _ in got] == \
               [(e["path_score"], e["region"], e["ops"], e["vulgar"]) for e in rec["subopt"]], rec["id"]
        rounds += len(got)
    assert rounds > len(load_set(name))                      # the loop went round


@pytest.mark.parametrize("name", CLI_SETS)
def test_oracle_matches_the_reference_binary_s_alignments(lib, name):
    """The pairs the reference binary aligned, on the strands it chose: score, region and transition ids."""
    data, model = load_cli(name)
    assert data["pairs"]
    for pair in data["pairs"]:
        q, t = (s.encode() for s in strand_seqs(pair))
        assert oracle_lib.find_score(model.c, model.params, q, t) == pair["score"], pair["id"]
        got = oracle_lib.find_path(model.c, model.params, q, t, dpmemory=32)
        assert (got["score"], got["region"], got["ops"]) == (pair["score"], pair["region"], pair["ops"]), pair["id"]


def _refdump(model_type, cases, dpmemory, flags):
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as f:
        for c in cases:                  # (a fourth entry: the query's annotated CDS (start, length), the reference's --annotation)
            f.write("%s\t%s\t%s" % c[:3] + ("\t%d:%d" % c[3] if len(c) > 3 else "") + "\n")
        path = f.name
    try:
        out = subprocess.run([REFDUMP, "--cmd", "golden", "--model", model_type, "--input", path, "-D", str(dpmemory)] + list(flags),
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    finally:
        os.unlink(path)
    recs = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert [r["id"] for r in recs] == [c[0] for c in cases]
    return recs


def _compare_with_refdump(model_type, point, dpm, pairs):
    """refdump over the pairs at one parameter point and -D dpm: the oracle's score and path must equal every record."""
    model = point_model(model_type, point)
    cases = [("p%03d" % n, q, t) for n, (q, t) in enumerate(pairs)]
    recs = _refdump(model_type, cases, dpm, ALL_POINTS[point])
    for rec, (_, q, t) in zip(recs, cases):
        q, t = q.encode(), t.encode()
        assert oracle_lib.find_score(model.c, model.params, q, t) == rec["score"], (point, dpm, rec["id"])
        a = oracle_lib.find_path(model.c, model.params, q, t, dpmemory=dpm, qid=rec["id"])
        if "path_score" not in rec:
            assert a is None, (point, dpm, rec["id"])
        else:
            assert a == expected(rec), (point, dpm, rec["id"], len(q), len(t))


@pytest.mark.parametrize("k", BANDS)
@pytest.mark.parametrize("model_type", sorted(EDGE_POINTS))
def test_generated_bands_cross_their_boundary(lib, model_type, k):
    """The condition of codon_cases.edge_pairs, decided by the oracle alone (so it is checked wherever the suite runs): among
    the alignments of band k, over its parameter points, a transition of every query advance the model has goes from a row
    below 256 k to a row at or above it -- for ungapped:trans landing 0, 1 and 2 rows past it -- and at every single point an
    advance of 3 does; so it is with the rows counted from the alignment's start, and coding2coding takes each of its six
    events at a row 256 k - 3 ... 256 k + 3 (codon_cases.band_shows)."""
    pairs = edge_pairs(model_type, k, band_rng(model_type, k))
    if k == "small":
        assert sorted(len(q) for q, _ in pairs) == list(range(1, 14)) and all(1 <= len(t) <= 20 for _, t in pairs)
        model = point_model(model_type, "default")
        alns = [oracle_lib.find_path(model.c, model.params, q.encode(), t.encode()) for q, t in pairs]
        assert sum(a is not None and a["score"] > 0 for a in alns) >= 6 and any(a is None or a["score"] == 0 for a in alns)
        return
    b = STRIP * k
    assert {len(q) for q, _ in pairs} == set(range(b - 2, b + 4))
    assert all(40 <= len(t) - len(q) <= 150 for q, t in pairs), [len(t) - len(q) for q, t in pairs]
    alns = {}
    for point in EDGE_POINTS[model_type]:
        model = point_model(model_type, point)
        alns[point] = [oracle_lib.find_path(model.c, model.params, q.encode(), t.encode()) for q, t in pairs]
    missing = band_shows(model_type, k, alns)
    assert missing is None, (model_type, k, missing)


needs_refdump = pytest.mark.skipif(not os.path.exists(REFDUMP),
                                   reason="oracle/_ref/refdump is built by build() where the reference tree is")


@needs_refdump
@pytest.mark.parametrize("dpm", [32, 0])
@pytest.mark.parametrize("nth_point", [0, 1])
@pytest.mark.parametrize("k", BANDS)
@pytest.mark.parametrize("model_type", sorted(EDGE_POINTS))
def test_live_bands_against_the_reference(lib, model_type, k, nth_point, dpm):
    """The bands the device tests use, at their parameter points, through the reference itself (its interpreted Viterbi takes
    seconds at four strips: one point and one -D per case)."""
    pairs = edge_pairs(model_type, k, band_rng(model_type, k))
    _compare_with_refdump(model_type, EDGE_POINTS[model_type][nth_point], dpm, pairs)


@needs_refdump
@pytest.mark.parametrize("dpm", [32, 0])
def test_live_band_at_a_penalty_of_3e8(lib, dpm):
    """--frameshift -350000000, the point at which the engine drops its local-scope shortcut: the band of the first strip edge."""
    _compare_with_refdump("coding2coding", "huge", dpm, edge_pairs("coding2coding", 1, band_rng("coding2coding", 1)))


@needs_refdump
@pytest.mark.parametrize("dpm", [32, 0])
@pytest.mark.parametrize("point", sorted(POINTS))
@pytest.mark.parametrize("model_type", sorted(EDGE_POINTS))
def test_live_fuzz_pairs_against_the_reference(lib, model_type, point, dpm):
    """codon_cases.fuzz_pair (one to five strips, second copies, ambiguity codes, lower case) at the three parameter points."""
    rng = random.Random(31 + len(model_type))
    pairs = {p: [fuzz_pair(rng) for _ in range(8)] for p in sorted(POINTS)}
    strips = {len(q) // STRIP + 1 for ps in pairs.values() for q, _ in ps}
    assert {1, 2, 3, 5} <= strips, strips
    _compare_with_refdump(model_type, point, dpm, pairs[point])


@needs_refdump
@pytest.mark.parametrize("dpm", [32, 0])
def test_live_annotation_veto_against_the_reference(lib, dpm):
    """--annotation on coding2coding (match.c:513-519): outside the query's annotated CDS, and inside it off its frame, no 3:3
    match.  The device refuses an annotated codon batch, so this branch of the oracle's calc is pinned here alone: CDS in each of
    the three frames, from the query's start, in its middle and to its end, one codon long, and longer than the query has left."""
    model = point_model("coding2coding", "default")
    pairs = edge_pairs("coding2coding", 1, band_rng("coding2coding", 1))
    cds = [(0, 120), (1, 90), (2, 252), (100, 159), (101, 3), (30, 60), (62, 190), (3, 251), (200, 59)]
    cases = [("a%03d" % n, q, t, c) for n, ((q, t), c) in enumerate(zip(pairs, cds))]
    assert len(cases) == len(cds) and {c[0] % 3 for c in cds} == {0, 1, 2}
    recs = _refdump("coding2coding", cases, dpm, [])
    changed = 0
    try:
        for rec, (_, q, t, c) in zip(recs, cases):
            q, t = q.encode(), t.encode()
            oracle_lib.set_annotation(None)
            plain = oracle_lib.find_score(model.c, model.params, q, t)
            oracle_lib.set_annotation(list(c))
            assert oracle_lib.find_score(model.c, model.params, q, t) == rec["score"], (dpm, rec["id"])
            changed += plain != rec["score"]
            a = oracle_lib.find_path(model.c, model.params, q, t, dpmemory=dpm, qid=rec["id"])
            if "path_score" not in rec:
                assert a is None, (dpm, rec["id"])
            else:
                assert a == expected(rec), (dpm, rec["id"])
    finally:
        oracle_lib.set_annotation(None)
    assert changed >= 6                         # the annotation is what decides these records
