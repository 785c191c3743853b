"""c4gpu_wordtab_build -- the seeder's word table built on the device from the queries themselves, word neighbourhoods included
(Seeder_insert_query seeder.c:478-558, wordhood.c) -- against what the reference's own automaton held (every record of
tests/golden/seeds_*.jsonl and wordtab_*.jsonl: the table word for word and emission for emission, the scan of the record's
target on it call for call, c4gpu_seed_extend on it HSP for HSP) and, on the edge inputs of tests/wordtab_cases.py, against the
plain-Python rules of tests/wordtab_model.py (pinned on the same records in tests/test_wordtab_model.py)."""
import ctypes as C

import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
import seed_fused_cases as sf
import wordtab_cases as wc
import wordtab_model as wm

pytestmark = pytest.mark.gpu

RECORDS = wm.all_records()
SETS = sorted({name for name, _, _ in RECORDS})


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def params():
    return ex.default_params()


def test_the_records_are_there():
    assert len(SETS) >= 12 and len(RECORDS) >= 30


@pytest.mark.parametrize("name", SETS)
def test_records(eng, params, name):
    """The built table is the reference's; scanning the record's target on it makes the reference's HSPset_seed_hsp calls in
    order; c4gpu_seed_extend keeps on it what it keeps on a table made from the record by c4gpu_wordtab_create."""
    kept = 0
    for set_name, flags, rec in RECORDS:
        if set_name != name:
            continue
        exp = wm.record_table(rec)
        with eng.wordtab_build(*wm.record_input(rec, flags)) as tab:
            codes, emit_first, emits = tab.export()
            assert codes == exp["codes"], rec["id"]
            assert emit_first == exp["emit_first"], rec["id"]
            assert emits == exp["emits"], rec["id"]
            assert tab.stats["n_words"] == len(codes) and tab.stats["n_emits"] == len(emits)
            hits, _ = eng.seed_scan(rec["width"], rec["wordlen"], tab, bytes(rec["symbols"]))
            assert [[emits[e][0], emits[e][1], pos - rec["tpos_modifier"]] for pos, e in hits] == rec["expected"], rec["id"]
            dropoff, threshold = sf.points(rec["match"])["default"]
            pairs = [(q, rec["target"]) for q in rec["queries"]]
            words, rec_emits = sf.record_table(rec)
            tail = ([bytes(rec["symbols"])], 1, [0], rec["tpos_modifier"], rec["wordlen"], dropoff, threshold)
            first_a, first_b = [], []
            got = eng.seed_extend(params, rec["match"], pairs, rec["width"], rec["wordlen"], tab, None, *tail, first_hits=first_a)
            ref = eng.seed_extend(params, rec["match"], pairs, rec["width"], rec["wordlen"], words, rec_emits, *tail, first_hits=first_b)
            assert got == ref and first_a == first_b, rec["id"]
            assert ref[1]["n_hits"] == len(rec["expected"]) > 0
            kept += ref[1]["n_kept"]
    assert kept > 0


def test_export_of_a_created_table(eng):
    """c4gpu_wordtab_export also serves a table made by c4gpu_wordtab_create + c4gpu_wordtab_set_emissions."""
    rec = wm.load("seeds_protein2protein")[0]
    words, emits = sf.record_table(rec)
    tab = ex._wordtab(eng.ctx, rec["width"], rec["wordlen"], words)
    try:
        with pytest.raises(ex.C4GpuError, match="no emissions set"):
            ex._wordtab_export(eng.ctx, tab)
        ce = (_abi.SeedEmit * len(emits))(*[_abi.SeedEmit(p, q) for p, q in emits])
        assert ex._lib().c4gpu_wordtab_set_emissions(tab, ce, len(emits)) == 0
        codes, emit_first, out = ex._wordtab_export(eng.ctx, tab)
    finally:
        ex._lib().c4gpu_wordtab_destroy(tab)
    assert codes == [c for c, _ in words] and out == [tuple(e) for e in emits]
    assert [b - a for a, b in zip(emit_first, emit_first[1:])] == [n for _, n in words]


def _against_the_model(eng, case):
    exp = case.model()
    with eng.wordtab_build(*case.args()) as tab:
        codes, emit_first, emits = tab.export()
        assert codes == exp["codes"], case.name
        assert emit_first == exp["emit_first"], case.name
        assert emits == exp["emits"], case.name
        st = tab.stats
        assert (st["n_occurrences"], st["n_seeded_words"], st["n_words"], st["n_emits"]) == \
               (exp["n_occurrences"], exp["n_seeded_words"], len(exp["codes"]), len(exp["emits"])), case.name
        assert st["n_links"] == (exp["n_links"] if case.scores is not None else 0), case.name
        hits, _ = eng.seed_scan(case.width, case.wordlen, tab, case.scan)
        assert hits == wc.scan_hits(case, exp), case.name
    return exp, hits


@pytest.mark.parametrize("case", wc.empties(), ids=lambda c: c.name)
def test_nothing_to_build_from(eng, params, case):
    exp, hits = _against_the_model(eng, case)
    assert exp["codes"] == [] and hits == []
    with eng.wordtab_build(*case.args()) as tab:                 # and c4gpu_seed_extend finds nothing on it
        got, stats = eng.seed_extend(params, "dna2dna", [("ACGTACGTACGT", "ACGTACGTACGT")], case.width, case.wordlen, tab, None,
                                     [case.scan], 1, [0], case.wordlen - 1, case.wordlen, 30, 10)
        assert got == [] and stats["n_hits"] == 0


@pytest.mark.parametrize("case", wc.edges(), ids=lambda c: c.name)
def test_edges_against_the_model(eng, case):
    exp, hits = _against_the_model(eng, case)
    assert exp["codes"] and hits


def test_no_score_table_means_no_neighbourhoods(eng):
    c = wc.many_links()
    c.scores = None
    exp, _ = _against_the_model(eng, c)
    assert all(not s for s in exp["sources"])


def test_two_builds_give_the_same_bytes(eng):
    for case in (wc.all_neighbours(), wc.many_links(), wc.wide_codes()):
        outs = []
        for _ in range(2):
            with eng.wordtab_build(*case.args()) as tab:
                outs.append(tab.export())
        assert outs[0] == outs[1], case.name


def test_refusals(eng):
    """Each returns NULL with a message before anything is launched; the context builds a table afterwards."""
    s = wc.flat(5, 5, -4)
    with pytest.raises(ex.C4GpuError, match="does not fit 63 bits"):
        eng.wordtab_build(25, 14, [bytes([1] * 20)], [(0, 1, 0)])
    with pytest.raises(ex.C4GpuError, match="does not fit 63 bits"):
        eng.wordtab_build(255, 8, [bytes([1] * 20)], [(0, 1, 0)])
    with pytest.raises(ex.C4GpuError, match="bad shape"):
        eng.wordtab_build(5, 0, [bytes([1] * 20)], [(0, 1, 0)])
    with pytest.raises(ex.C4GpuError, match="bad shape"):
        eng.wordtab_build(256, 3, [bytes([1] * 20)], [(0, 1, 0)])
    with pytest.raises(ex.C4GpuError, match="negative pair"):
        eng.wordtab_build(5, 4, [bytes([1, 2, 3, 4])], [(-1, 1, 0)], scores=s, threshold=9)
    with pytest.raises(ex.C4GpuError, match="scale below 1"):
        eng.wordtab_build(5, 4, [bytes([1, 2, 3, 4])], [(0, 0, 0)])
    with pytest.raises(ex.C4GpuError, match="beyond"):
        eng.wordtab_build(5, 4, [bytes([1, 2, 3, 4])], [(0, 1, 0)], scores=wc.flat(5, 1 << 21, 0), threshold=9)
    # a negative length cannot be said through the Python call
    strs = (C.c_char_p * 1)(bytes([1, 2, 3, 4]))
    lens = (C.c_int32 * 1)(-4)
    src = (_abi.WordSource * 1)(_abi.WordSource(0, 1, 0))
    assert not ex._lib().c4gpu_wordtab_build(eng.ctx, 5, 4, strs, lens, src, 1, None, 0, 1, None)
    assert b"negative length" in ex._lib().c4gpu_last_error()
    assert not ex._lib().c4gpu_wordtab_build(eng.ctx, 5, 4, strs, lens, src, -1, None, 0, 1, None)
    with eng.wordtab_build(5, 4, [bytes([1, 2, 3, 4])], [(0, 1, 0)], scores=s, threshold=9) as tab:
        assert tab.stats["n_words"] == 13 and tab.stats["n_links"] == 12
