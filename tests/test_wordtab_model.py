"""tests/wordtab_model.py -- the word table's rules in plain Python (include/c4gpu.h: c4gpu_wordtab_build) -- against what the
reference's own automaton held: the words of every seeds_*.jsonl record (tools/make_golden.py) and every wordtab_*.jsonl record
(tools/make_wordtab_golden.py), read off its trie / leaf table by oracle/refdump.c --cmd seeds.  And the edge inputs of
tests/wordtab_cases.py: that each has, on the model, the property the device test uses it for."""
import pytest

import wordtab_cases as wc
import wordtab_model as wm

# the flags of the six existing sets (tools/make_golden.py:928-932)
SEEDS_FLAGS = {
    "seeds_dna2dna": (),
    "seeds_dna2dna_w9": ("--dnawordlen", "9"),
    "seeds_dna2dna_compact": ("--forcefsm", "compact"),
    "seeds_dna2dna_hood": ("--dnawordlen", "8", "--dnawordlimit", "5"),
    "seeds_protein2protein": ("--proteinwordlimit", "2"),
    "seeds_protein2protein_compact": ("--proteinwordlimit", "1", "--forcefsm", "compact"),
}
WORDTAB_SETS = wm.wordtab_sets()


def test_flag_table():
    assert wm.SEEDS_FLAGS == SEEDS_FLAGS
    assert len(WORDTAB_SETS) >= 6


def _check(rec, flags):
    # the column map first: the record's target went through the reference's own traversal filter
    col = wm.columns(rec["match"], rec["automaton"])
    assert [col.get(ch.upper(), 0) for ch in rec["target"]] == rec["symbols"], rec["id"]
    got, exp = wm.build(*wm.record_input(rec, flags)), wm.record_table(rec)
    assert got["codes"] == exp["codes"], rec["id"]
    assert got["own"] == exp["own"], rec["id"]
    assert got["sources"] == exp["sources"], rec["id"]
    assert got["emit_first"] == exp["emit_first"] and got["emits"] == exp["emits"], rec["id"]
    return got


@pytest.mark.parametrize("name", sorted(SEEDS_FLAGS))
def test_model_reproduces_the_seeds_sets(name):
    recs = wm.load(name)
    assert recs
    for rec in recs:
        _check(rec, SEEDS_FLAGS[name])


@pytest.mark.parametrize("name", WORDTAB_SETS)
def test_model_reproduces_the_wordtab_sets(name):
    recs = wm.load(name)
    assert recs
    for rec in recs:
        got = _check(rec, rec["flags"])
        assert got["n_links"] > 0 and len(rec["queries"]) <= 8 and max(len(q) for q in rec["queries"]) <= 60


def test_the_wordtab_sets_cover_what_they_are_for():
    recs = {name: wm.load(name) for name in WORDTAB_SETS}
    flags = {name: wm.record_flags(rs[0]["flags"]) for name, rs in recs.items()}
    every = [r for rs in recs.values() for r in rs]
    assert {r["automaton"] for r in every} == {"fsm", "vfsm"}
    assert any(f["limit"] is None for f in flags.values())                                   # the default protein limit
    assert any(not f["use_dropoff"] for f in flags.values())
    assert any(r["match"] == "dna2dna" and sum(len(w[2]) for w in r["words"]) for r in every)
    assert max(len(w[2]) for r in every for w in r["words"]) >= 3                            # several neighbour sources
    for r in every:
        assert any(len({q for q, _ in w[1]}) > 1 for w in r["words"])                        # queries that share words
        assert any(wm.columns(r["match"], r["automaton"]).get(ch, 0) == 0 for q in r["queries"] for ch in q)     # a reset
        assert any(len(q) < r["wordlen"] for q in r["queries"])


# ---- the edge inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.empties(), ids=lambda c: c.name)
def test_empties_have_no_words(case):
    t = case.model()
    assert t["codes"] == [] and t["emits"] == [] and t["emit_first"] == [0]
    assert wc.scan_hits(case, t) == []


def test_wordlen_one():
    c = wc.wordlen_one()
    t = c.model()
    assert c.wordlen == 1 and t["n_links"] > 0 and any(not o for o in t["own"])              # a word with neighbour lists only


def test_identical_queries_alternate_pairs():
    t = wc.identical_queries().model()
    k = t["codes"].index(wm.code_of(5, (1, 2, 3, 4)))
    assert t["own"][k] == [(1, 4), (1, 0), (0, 4), (0, 0)]                                   # g descending


def test_neighbour_across_queries():
    t = wc.neighbour_across_queries().model()
    k = t["codes"].index(wm.code_of(5, (1, 2, 3, 4)))
    assert t["emits"][t["emit_first"][k]:t["emit_first"][k + 1]] == [(0, 0), (1, 0)]         # own first, then the neighbour's
    k = t["codes"].index(wm.code_of(5, (1, 2, 3, 3)))
    assert t["emits"][t["emit_first"][k]:t["emit_first"][k + 1]] == [(1, 0), (0, 0)]


def test_more_than_64_sources_and_more_than_two_sort_tiles():
    t = wc.all_neighbours().model()
    assert len(t["codes"]) == 125 and all(len(s) == 124 for s in t["sources"])               # > 64: past a wave's width
    assert t["n_links"] == 125 * 124 > 2 * 2048
    t = wc.many_links().model()
    assert t["n_links"] > 2 * 2048


def test_codes_at_or_above_2_to_32():
    t = wc.wide_codes().model()
    seeded = [c for c, o in zip(t["codes"], t["own"]) if o]
    assert any(c >= 1 << 32 for c in seeded) and any(c < 1 << 32 for c in seeded)
    assert any(c >= 1 << 32 for c, o in zip(t["codes"], t["own"]) if not o)                  # neighbour-only words up there too
    assert max(t["codes"]) < 25 ** 7


def test_prefix_failure_under_a_passing_total():
    c = wc.prefix_failure()
    t = c.model()
    found = 0
    for s in c.strings:
        for p in range(len(s) - c.wordlen + 1):
            w = tuple(s[p:p + c.wordlen])
            reach = set(wm.hood(c.width, c.wordlen, w, c.scores, c.threshold, c.use_dropoff))
            for a in range(1, c.width):
                for b in range(1, c.width):
                    for d in range(1, c.width):
                        n = (a, b, d)
                        if n not in reach and wm.total_passes(c.wordlen, w, n, c.scores, c.threshold, c.use_dropoff):
                            found += 1
                            k = t["codes"].index(wm.code_of(c.width, n)) if wm.code_of(c.width, n) in t["codes"] else None
                            assert k is None or wm.code_of(c.width, w) not in t["sources"][k]
    assert found > 0
    assert (2, 2, 3) not in wm.hood(c.width, c.wordlen, (3, 1, 3), c.scores, c.threshold, True)
    assert wm.total_passes(c.wordlen, (3, 1, 3), (2, 2, 3), c.scores, c.threshold, True)


def test_absolute_threshold_above_a_self_score():
    c = wc.absolute_threshold()
    assert not c.use_dropoff
    reach = wm.hood(c.width, c.wordlen, (1, 1, 1), c.scores, c.threshold, False)
    assert (1, 1, 1) not in reach and (5, 1, 1) in reach
    t = c.model()
    k = t["codes"].index(wm.code_of(c.width, (5, 1, 1)))
    assert t["own"][k] == [] and wm.code_of(c.width, (1, 1, 1)) in t["sources"][k]


def test_translated_frames_positions():
    c = wc.translated_frames()
    t = c.model()
    assert {q % 3 for _, q in t["emits"]} == {0, 1, 2} and {p for p, _ in t["emits"]} == {0}
    assert any(len({q % 3 for _, q in o}) > 1 for o in t["own"])                             # a word two frames share
