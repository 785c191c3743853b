"""The yardstick of c4gpu_seed_extend pinned on the oracle (CPU): seed_fused_cases.replay over every reference-generated seeder
record (tests/golden/seeds_*.jsonl) equals oracle_lib.hsp_set query by query, at the dropoff / threshold of hsp_<match>.jsonl and
of the lowered set; the records hold what makes the GPU tests bite (skipped seeds, extended seeds below the threshold, chains
that keep several HSPs); the generated cases have the properties their names claim."""
import pytest

import exonerate_amd as ex
import oracle_lib
import seed_fused_cases as sf
from test_oracle_seed import SEED_SETS, load_seed_set

RECORDS = [(name, k) for name in SEED_SETS for k in range(len(load_seed_set(name)))]


@pytest.fixture(scope="module")
def params():
    return ex.default_params()


def test_the_engine_has_the_fused_call():
    assert hasattr(ex.Engine, "seed_extend")


def test_all_records_are_here():
    assert len(RECORDS) == 25


_replayed = {}


def _replay(params, name, k, point, source="expected"):
    key = (name, k, point, source)
    if key not in _replayed:
        rec = load_seed_set(name)[k]
        dropoff, threshold = sf.points(rec["match"])[point]
        calls = rec["expected"] if source == "expected" else oracle_lib.seed_walk(rec)
        detail = {}
        kept, stats = sf.replay(params, rec["match"], rec["queries"], rec["target"], calls, rec["wordlen"], dropoff, threshold,
                                detail=detail)
        _replayed[key] = (rec, kept, stats, detail)
    return _replayed[key]


@pytest.mark.parametrize("point", ["default", "low"])
@pytest.mark.parametrize("name,k", RECORDS)
def test_replay_is_the_oracles_hsp_set(params, name, k, point):
    rec, kept, stats, _ = _replay(params, name, k, point)
    dropoff, threshold = sf.points(rec["match"])[point]
    total = 0
    for qi, q in enumerate(rec["queries"]):
        seeds = [(qs, ts) for x, qs, ts in rec["expected"] if x == qi]
        exp = oracle_lib.hsp_set(params, rec["match"], q.encode(), rec["target"].encode(), rec["wordlen"], dropoff, threshold, seeds)
        assert [h for _, x, h in kept if x == qi] == exp, (rec["id"], qi)
        total += len(exp)
    assert stats["n_kept"] == total and stats["n_hits"] == len(rec["expected"])
    assert stats["n_extended"] == stats["n_below"] + stats["n_kept"]
    assert [s for s, _, _ in kept] == sorted(s for s, _, _ in kept)


@pytest.mark.parametrize("name,k", RECORDS)
def test_replay_over_the_oracles_walk_gives_the_same(params, name, k):
    assert _replay(params, name, k, "default", "walk")[1:3] == _replay(params, name, k, "default")[1:3]
    assert _replay(params, name, k, "low", "walk")[1:3] == _replay(params, name, k, "low")[1:3]


@pytest.mark.parametrize("point", ["default", "low"])
@pytest.mark.parametrize("name,k", RECORDS)
def test_every_record_has_skipped_seeds(params, name, k, point):
    _, _, stats, _ = _replay(params, name, k, point)
    assert 0 < stats["n_extended"] < stats["n_hits"]


@pytest.mark.parametrize("name", [n for n in SEED_SETS if "dna2dna" in n])
def test_extended_seeds_fall_below_the_default_dna_threshold(params, name):
    """(The oracle counts 8, 6, 16 and 13 such seeds in seeds_dna2dna, _compact, _hood and _w9.)"""
    below = sum(_replay(params, name, k, "default")[2]["n_below"] for k in range(len(load_seed_set(name))))
    assert below >= 1


def test_chains_that_keep_several_hsps_at_the_lowered_point(params):
    """(The oracle finds 9 such records, all of them DNA.)"""
    n = 0
    for name, k in RECORDS:
        detail = _replay(params, name, k, "low")[3]
        n += any(v >= 2 for v in detail["entry_kept"].values())
    assert n >= 3


def test_case_one_diagonal_two_hsps(params):
    c = sf.case_one_diagonal_two_hsps()
    kept, stats = c.replay(params)
    assert stats["n_kept"] == 2 and stats["n_extended"] < stats["n_hits"]
    (_, _, a), (_, _, b) = kept
    assert a[1] - a[0] == b[1] - b[0] == 0 and a[:3] == [0, 0, 22] and b[:3] == [37, 37, 23]


def test_case_shared_entry_differs_from_a_diagonal_key(params):
    c = sf.case_shared_entry_across_diagonals()
    q = c.queries[0]
    assert len(q) == 30 and q[20:30] == q[10:20] and len(c.target) == 150
    by_section, by_diagonal = c.replay(params), c.replay(params, key="diagonal")
    assert by_section != by_diagonal
    assert by_section[1]["n_extended"] < by_diagonal[1]["n_extended"]
    assert {ts % 3 for _, _, ts in c.calls} == {0}            # every hit in the first frame string ...
    assert len({ts - 3 * qs for _, qs, ts in c.calls}) >= 3   # ... on the main diagonal and the ones 30 bases either side


def test_case_negative_section(params):
    import math
    c = sf.case_negative_section()
    neg = [k for k, (_, qs, ts) in enumerate(c.calls) if int(math.fmod(ts - 3 * qs + 30, 30)) < 0]
    assert neg and [20, 3] in [x[1:] for x in c.calls]
    kept, stats = c.replay(params)
    assert all(k in {s for s, _, _ in kept} for k in neg)      # (six identical residues: over the threshold, never skipped)


@pytest.mark.parametrize("name", [s[0] for s in sf.EDGE_SHAPES])
def test_case_edges(params, name):
    c = sf.case_edge(name)
    tlen, qlens = [(t, q) for n, t, q in sf.EDGE_SHAPES if n == name][0]
    assert len(c.target) == len(c.strings[0]) == tlen and [len(q) for q in c.queries] == qlens
    assert sum(qlens) in (255, 257, 65535, 65537)
    kept, stats = c.replay(params)
    assert stats["n_kept"] >= 5 and stats["n_extended"] < stats["n_hits"]
    assert {0, len(qlens) - 1} <= {q for _, q, _ in kept}      # first and last pair: lowest and highest slot numbers


def test_cases_nothing_to_report(params):
    cases = sf.cases_nothing_to_report()
    assert len(cases) == 3
    for c in cases:
        assert c.calls == [] and c.words
    assert len(cases[0].strings[0]) < cases[0].wordlen and set(cases[1].strings[0]) == {0}
