"""Every kernel form of the one-row-advance families -- affine (four scopes, DNA and protein), ner, est2genome, protein2dna,
protein2genome -- on the MI355X against the CPU oracle at its own strip, workgroup, super-strip, chunk and dump edges
(tests/edge_cases.py; tests/test_edge_cases.py proves on the oracle alone that the bands put something on those edges and pins
the kernel each case expects).  One form per case: the case sets the form's switches, runs find_score and find_path (dpmemory 32:
the PATH kernels; dpmemory 0: REGION, CKPT and the PATH continuations) over the band's batch, compares EVERY pair with the oracle
-- score, region, op list, sugar / cigar / vulgar -- and asserts from C4GPU_TRACE that the kernel it means to test served (the
name comes from the kernel choice linked against the kernel table, at the case's own batch; tests/test_edge_cases.py pins those
names to its literal tables COVERAGE_32 and COVERAGE_SEEDED, which list every form, kernel and band).
Integer work and text: every comparison is exact.  Nothing here needs the reference binaries."""
import re

import pytest

import exonerate_amd as ex
import edge_cases as ec
from test_gpu_codon_oracle import _kernels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


def _launched(err):
    """Every kernel a traced call names: the launches (_kernels), the seeded passes, the device route's continuation kernels and
    its packed checkpoint kernels."""
    names = set(_kernels(err))
    names.update(re.findall(r"seeded pass \d with kernel (k\w+)", err))
    for line in err.splitlines():
        if "fused: kernels" in line or "fused: packed checkpoint kernels" in line:
            names.update(re.findall(r"\b(k[a-z0-9]*_[a-z0-9_]+)", line.split("fused:")[1]))
    return names


def _groups(family, band, only=None):
    """The band's pairs (those of `only`) by parameter point: [(model, [index of each pair])] -- one call each."""
    by_point = {}
    for n, p in enumerate(ec.band_pairs(family, band)):
        if only is None or n in only:
            by_point.setdefault(p.get("point", "default"), []).append(n)
    return [(point, ec.family_model(family, point), idx) for point, idx in sorted(by_point.items(), key=lambda kv: kv[0] != "default")]


def _run_band(eng, capfd, family, band, dpms=(32, 0), score=True, only=None):
    """find_score and find_path over the band's batch, every pair against the oracle; returns {"score" / dpmemory: (kernels the
    call of the default parameter point launched, its trace)}."""
    pairs = ec.band_pairs(family, band)
    seen = {}
    for point, model, idx in _groups(family, band, only):
        batch = [(pairs[n]["q"], pairs[n]["t"]) for n in idx]
        capfd.readouterr()
        if score:
            got = eng.find_score(model, batch)
            exp = ec.oracle_scores(family, band)
            err = capfd.readouterr().err
            for n, g in zip(idx, got):
                assert g == exp[n], (family, band, point, "score", n, len(pairs[n]["q"]), len(pairs[n]["t"]), pairs[n]["claims"])
            seen.setdefault("score", (_launched(err), err))
        for dpm in dpms:
            got = [a.as_dict() if a is not None else None for a in eng.find_path(model, batch, dpmemory=dpm)]
            exp = ec.oracle_paths(family, band, dpm)
            err = capfd.readouterr().err
            for n, g in zip(idx, got):
                assert g == exp[n], (family, band, point, dpm, n, len(pairs[n]["q"]), len(pairs[n]["t"]), pairs[n]["claims"])
            seen.setdefault(dpm, (_launched(err), err))
    return seen


def _setenv(monkeypatch, env):
    monkeypatch.setenv("C4GPU_TRACE", "1")
    for k, v in env.items():
        monkeypatch.setenv("C4GPU_" + k, v)


def _default_lengths(family, band):
    return [len(p["q"]) for p in ec.band_pairs(family, band) if p.get("point", "default") == "default"]


# ---- the 32-bit forms ----------------------------------------------------------------------------------------------------------
# est2genome's 32-bit cases keep the packed passes out (the device route would serve its checkpoint jobs on the packed kernel)
KEEP_32 = {"est2genome": {"PK16": "0", "CK16": "0"}}
CASES32 = [(family, form, band) for family in ec.FAMILIES for form in ec.FORMS32 for band in ec.form32_bands(family, form)]


@pytest.mark.parametrize("family, form, band", CASES32, ids=["%s-%s-%d" % (f, m, b[0]) for f, m, b in CASES32])
def test_32_bit_forms_at_their_row_edges(eng, monkeypatch, capfd, family, form, band):
    """One form of edge_cases.FORMS32 at one of its own row boundaries: queries of b - 2 ... b + 2 rows, alignments that begin at
    rows b - 1 ... b + 1, every event of the family starting at rows b - 1 and b, ties between end cells on either side of b."""
    env = dict(ec.FORMS32[form][0], **KEEP_32.get(family, {}))
    _setenv(monkeypatch, env)
    seen = _run_band(eng, capfd, family, band)
    expect = ec.form_launches(family, form, _default_lengths(family, band))
    about = ec.FORMS32[form][1]
    where = {"score": "score", "region": 0, "path": 32, "ckpt_cont": 0, "path_cont": 0}
    for what in about:
        if what == "region" and ec.FAMILIES[family][0] == "affine:global":
            continue                                        # (a global model has no region pass: optimal.c:135)
        assert expect[what]["name"] in seen[where[what]][0], (what, expect[what]["name"], sorted(seen[where[what]][0]))
    tag = "_%s_" % ec.kernel_family(family)
    assert all(tag in n for names, _ in seen.values() for n in names), seen
    if form in ("host-route", "device-route"):
        assert ("pairs finished on the device route" in seen[0][1]) == (form == "device-route"), seen[0][1][-1500:]
    if form == "one-wave":
        assert not any(n.startswith("kmw") for names, _ in seen.values() for n in names), seen


@pytest.mark.parametrize("family", sorted(ec.FAMILIES))
def test_lengths_0_to_3_on_either_side(eng, monkeypatch, capfd, family):
    """Queries and targets of 0 ... 3 residues (translated targets: 0 ... 5 nucleotides in all three frames, fewer columns than
    the largest target advance), an empty query beside a non-empty one in the same batch."""
    _setenv(monkeypatch, KEEP_32.get(family, {}))
    _run_band(eng, capfd, family, "small")


COL_ROWS = 530
CASES_COLS = [(family, form) for family in ec.FAMILIES for form in ("four-waves", "eight-waves")
              if ec.form32_bands(family, form)]


@pytest.mark.parametrize("family, form", CASES_COLS, ids=["%s-%s" % c for c in CASES_COLS])
def test_cooperating_waves_at_their_chunk_edges(eng, monkeypatch, capfd, family, form):
    """The cooperating-wave forms hand the bottom row on in chunks of 64 columns through a ring of 256: targets of c - 1, c and
    c + 1 columns and end cells at columns c - 1, c and c + 1 for c = 64 ... 320, introns that begin at c - 1 and end at c + 1."""
    env = dict(ec.FORMS32[form][0], **KEEP_32.get(family, {}))
    _setenv(monkeypatch, env)
    band = ("cols", COL_ROWS)
    seen = _run_band(eng, capfd, family, band)
    expect = ec.form_launches(family, form, _default_lengths(family, band))
    assert expect["score"]["waves"] > 1 and expect["score"]["name"] in seen["score"][0], (expect["score"], seen["score"][0])
    if ec.FAMILIES[family][0] != "affine:global":
        assert expect["region"]["waves"] > 1 and expect["region"]["name"] in seen[0][0], (expect["region"], seen[0][0])


# ---- the windowed region pass and the packed forms ----------------------------------------------------------------------------
def _run_seeded(eng, monkeypatch, capfd, form, band):
    family, env, about = ec.FORMS_SEEDED[form]
    _setenv(monkeypatch, env)
    pairs = ec.band_pairs(family, band)
    codes = len(set("".join(p["t"] for p in pairs)))
    for k, call in enumerate(ec.seeded_calls(form, band)):
        names, err = _run_band(eng, capfd, family, band, dpms=(0,), score=False, only=call)[0]
        lengths = [len(pairs[n]["q"]) for n in call
                   if pairs[n].get("point", "default") == "default" and len(pairs[n]["t"]) >= (4 << int(env["SEED_KSHIFT"]))]
        assert len(lengths) >= 2, lengths
        expect = ec.seeded_geometry(form, lengths, codes)
        for what in (about if k == 0 else ("seed1",)):     # (the second call of a split band: the form the choice turns to)
            if what == "ck16":
                line = [ln for ln in err.splitlines() if "fused: packed checkpoint kernels" in ln]
                assert line and expect[what]["name"] in line[0], (expect[what]["name"], line)
            else:
                line = [ln for ln in err.splitlines() if "seeded pass %s with kernel" % what[-1] in ln]
                assert line and line[0].split()[-1] == expect[what]["name"], (expect[what]["name"], line[:2], err[-1500:])


CASES_SEEDED = [(form, band) for form in ec.FORMS_SEEDED for band in ec.seeded_bands(form)]


def _band_id(band):
    return "c8-%d" % band[1][0] if band[0] == "c8" else "%s-%s" % band[:2] if isinstance(band[0], str) else str(band[0])


@pytest.mark.parametrize("form, band", CASES_SEEDED, ids=["%s-%s" % (f, _band_id(b)) for f, b in CASES_SEEDED])
def test_seeded_and_packed_forms_at_their_row_edges(eng, monkeypatch, capfd, form, band):
    """One form of edge_cases.FORMS_SEEDED -- the two-pass region search in 32 bits (est2genome on two and four window waves,
    protein2genome), each form of the packed score pass, each shape of the packed windows and of the packed checkpoint pass --
    at one of its own row boundaries, with a dump every 32 (64) columns: find_path at dpmemory 0, every pair against the oracle."""
    _run_seeded(eng, monkeypatch, capfd, form, band)


@pytest.mark.parametrize("form", sorted(ec.FORMS_SEEDED))
def test_seeded_and_packed_forms_at_dump_columns(eng, monkeypatch, capfd, form):
    """Every one of the same forms over the column band (edge_cases.seeded_col_band): end cells and target ends at c - 1, c and
    c + 1 for c = 64 ... 320 -- dump columns at a dump every 32 columns, chunk edges and the ring's wrap -- and introns that begin
    on c - 1 and end on c + 1, jumping over the dump column between; for the packed forms also an intron longer than the 15-bit
    length counter, for the six-row and the long form one query long enough to put the launch on them."""
    _run_seeded(eng, monkeypatch, capfd, form, ec.seeded_col_band(form))


# (switches, band and claim of job B): the score form by the batch's longest query, one window and one checkpoint shape each --
# a single wave, and two, four and eight cooperating waves
LANE_CASES = {
    "staged": (dict(ec._PACKED, WIN16="5", CK16="9"), ec.band_of(512, 520), ("event", "intron", 512)),
    "eight-waves": (dict(ec._PACKED, PK16_NW8="1", WIN16="6", CK16="6"), ec.band_of(512, 520), ("event", "intron", 512)),
    "six-rows": (dict(ec._PACKED, WIN16="8", CK16="5"), ec.band_of(1024, 520), ("event", "intron", 1024)),
    "long": (dict(ec._PACKED, WIN16="9", CK16="2"), ec.band_of(1536, 1542), ("event", "intron", 1536)),
}
LANE_SCORE_KERNEL = {"staged": "kpk16f", "eight-waves": "kpk16g", "six-rows": "kpk16h", "long": "kpk16j"}


@pytest.mark.parametrize("case", sorted(LANE_CASES))
def test_lane_halves_of_the_packed_forms_are_independent(eng, monkeypatch, capfd, case):
    """The packed forms put two unrelated jobs into the halves of one register.  Job A (an intron on row 255, a strip edge) beside
    job B (an intron on a row boundary of its own: other rows, other columns, other edges), in either half, beside itself,
    beside a filler, and in an odd batch: A's result is the oracle's each time, and so is every other job's; the score, window
    and checkpoint kernels are the ones the kernel choice names for each batch."""
    family = "est2genome"
    env, big, claim_b = LANE_CASES[case]
    _setenv(monkeypatch, env)
    model = ec.family_model(family)
    small = ec.band_of(256, 520)

    def pick(band, claim):
        n = next(n for n, p in enumerate(ec.band_pairs(family, band)) if claim in p["claims"])
        p = ec.band_pairs(family, band)[n]
        return (p["q"], p["t"]), ec.oracle_paths(family, band, 0)[n]

    a, exp_a = pick(small, ("event", "intron", 255))
    b, exp_b = pick(big, claim_b)
    filler, exp_f = pick(small, ("start", 257))
    assert exp_a is not None and exp_b is not None and len(a[0]) != len(b[0]) and len(a[1]) != len(b[1])
    served = set()
    for batch, exp in (([a, b], [exp_a, exp_b]), ([b, a], [exp_b, exp_a]), ([a, a], [exp_a, exp_a]),
                       ([a, filler], [exp_a, exp_f]), ([a, b, a], [exp_a, exp_b, exp_a])):
        capfd.readouterr()
        got = [x.as_dict() if x is not None else None for x in eng.find_path(model, batch, dpmemory=0)]
        err = capfd.readouterr().err
        expect = ec.launches_seeded(family, env, ("seed1", "seed2", "ck16"), [len(q) for q, _ in batch])
        for what in ("seed1", "seed2"):
            line = [ln for ln in err.splitlines() if "seeded pass %s with kernel" % what[-1] in ln]
            assert line and line[0].split()[-1] == expect[what]["name"], (expect[what]["name"], line[:2], err[-1500:])
        line = [ln for ln in err.splitlines() if "fused: packed checkpoint kernels" in ln]
        assert line and expect["ck16"]["name"] + " for %d," % len(batch) in line[0], (expect["ck16"]["name"], line)
        served.add(expect["seed1"]["name"])
        assert got == exp, [len(q) for q, _ in batch]
    assert LANE_SCORE_KERNEL[case] + "_est2genome" in served, served
