"""What makes tests/test_gpu_edges.py a test of the strip, workgroup, chunk and dump edges, decided on the CPU oracle's alignments
alone (no GPU): every band of tests/edge_cases.py shows what it is named for -- each event of the family with its transition
starting at rows b - 1 and b, alignments that begin at rows b - 1, b and b + 1, queries of b - 2 ... b + 2 rows, end cells and
target ends at columns c - 1, c and c + 1, introns that begin, end on and cover those columns, ties that exist (oracle scores of
the sub-problems) -- and, with the kernel choice linked against the real kernel table (tests/kernel_choice_sim.hip), which kernel
each (form, band) of the device tests expects: a change of a strip height or of the choice shows here first.  A band that does not
show a claim fails; nothing skips."""
import pytest

import edge_cases as ec
import kernel_choice_sim_lib as kc

FAMILIES = sorted(ec.FAMILIES)


def _bands_in_use():
    """Every (family, band) some case of tests/test_gpu_edges.py runs."""
    used = set()
    for family in FAMILIES:
        used.add((family, "small"))
        for form in ec.FORMS32:
            for band in ec.form32_bands(family, form):
                used.add((family, band))
            if form in ("four-waves", "eight-waves") and ec.form32_bands(family, form):
                used.add((family, ("cols", 530)))
    for form, (family, env, about) in ec.FORMS_SEEDED.items():
        for band in ec.seeded_bands(form):
            used.add((family, band))
        used.add((family, ec.seeded_col_band(form)))
    return sorted(used, key=repr)


BANDS = _bands_in_use()


@pytest.mark.parametrize("family, band", BANDS, ids=[repr(b).replace(" ", "") for b in BANDS])
def test_the_bands_put_their_events_on_their_boundaries(family, band):
    """Row origin: a band (b, pad_to, True) is proven against both origins -- its pairs align from query row 0, so row b of the
    query is row b of the alignment (score, region and window passes count the former, path, checkpoint and continuation passes
    the latter); a band (b, pad_to, False) against the query's own rows alone."""
    missing = ec.band_shows(family, band)
    assert missing is None, (family, band, missing)
    assert all(a is not None for a in ec.oracle_paths(family, band, 32)) or band == "small"


def test_a_band_whose_event_moved_two_rows_fails():
    """The proof notices an event two rows away from where its band claims it."""
    family, band = "est2genome", ec.band_of(256)
    pairs = ec.band_pairs(family, band)
    n = next(n for n, p in enumerate(pairs) if ("event", "intron", 255) in p["claims"])
    moved = dict(pairs[n], claims=[("event", "intron", 257)])
    aln = ec.oracle_paths(family, band, 32)[n]
    assert ec.pair_shows(ec.family_model(family), pairs[n], aln) is None
    assert "does not hold" in ec.pair_shows(ec.family_model(family), moved, aln)


def test_geometry_comes_from_the_kernel_table():
    """kernel_choice_sim_lib.geometry / form_geometry: KernelInfo::R, waves and hbm_carry of the chosen kernel, and the staged
    rows of the packed score pass."""
    g = kc.geometry((800, 24), {}, family=kc.FAMILY["est2genome"], mode=kc.SCORE, local=1, local_exact=1, cu_count=256)
    assert (g["name"], g["waves"], g["error"]) == ("kmw8_est2genome_score_local", 8, None) and g["R"] * 64 * g["waves"] == 1024
    g = kc.geometry((800, 24), {"MW": 0}, family=kc.FAMILY["est2genome"], mode=kc.SCORE, local=1, local_exact=1, cu_count=256)
    assert (g["name"], g["waves"]) == ("k_est2genome_score_local", 1)
    assert g["staged_rows"] == 4 * 64 * kc.form_geometry(kc.PK16, "est2genome", 5)["R"]
    assert g["staged_rows6"] == 4 * 64 * kc.form_geometry(kc.PK16, "est2genome", 7)["R"]
    assert kc.form_geometry(kc.WIN16, "est2genome", 4)["hbm_carry"] == 1
    assert kc.form_geometry(kc.PK16, "affine", 5)["name"] is None
    bad = kc.geometry((800, 24), {}, family=kc.FAMILY["est2genome"], mode=kc.CKPT, local=1, local_exact=1, cu_count=256)
    assert bad["name"] is None and bad["error"] == "no compiled kernel for this model/mode"
    assert ec.form_boundaries([kc.form_geometry(kc.CK16_ROOTED, "est2genome", 4)]) == {
        256: "strip of kck16r_est2genome_r4w2n4", 1024: "workgroup of kck16r_est2genome_r4w2n4 (carry rows through HBM)"}
    assert ec.form_boundaries([kc.form_geometry(kc.PK16, "est2genome", 9)]) == {
        384: "strip of kpk16j_est2genome", 1536: "workgroup of kpk16j_est2genome"}


# ---- the coverage table: (family, form) -> the kernels the form is about and the row boundaries its cases run at -------------------
COVERAGE_32 = {
    # est2genome: rows per lane 4 (one and four waves), 2 (eight waves), 1 (path), 3 (checkpoints)
    ("est2genome", "one-wave"): (["k_est2genome_score_local", "k_est2genome_region_local_pack", "k_est2genome_path",
                                  "k_est2genome_ckpt_cont_local", "k_est2genome_path_cont_local"], [64, 192, 256]),
    ("est2genome", "four-waves"): (["kmw_est2genome_score_local", "kmw_est2genome_region_local_pack"], [256, 1024]),
    ("est2genome", "eight-waves"): (["kmw8_est2genome_score_local", "kmw8_est2genome_region_local_pack"], [128, 1024]),
    ("est2genome", "general"): (["k_est2genome_score", "k_est2genome_region_pack"], [256]),
    ("est2genome", "two-slot"): (["kmw8_est2genome_region_local"], [128, 1024]),
    ("est2genome", "cont-masks"): (["k_est2genome_ckpt_cont", "k_est2genome_path_cont"], [64, 192]),
    ("protein2genome", "one-wave"): (["k_protein2genome_score_local", "k_protein2genome_region_local_pack", "k_protein2genome_path",
                                      "k_protein2genome_ckpt_cont_local", "k_protein2genome_path_cont_local"], [128]),
    ("protein2genome", "four-waves"): (["kmw_protein2genome_score_local", "kmw_protein2genome_region_local_pack"], [128, 512]),
    ("protein2genome", "eight-waves"): (["kmw8_protein2genome_score_local", "kmw8_protein2genome_region_local_pack"], [64, 512]),
    ("protein2genome", "general"): (["kmw_protein2genome_score", "kmw_protein2genome_region_pack"], [128, 512]),
    ("protein2genome", "two-slot"): (["kmw8_protein2genome_region_local"], [64, 512]),
    ("protein2genome", "cont-masks"): (["k_protein2genome_ckpt_cont", "k_protein2genome_path_cont"], [128]),
    ("protein2dna", "one-wave"): (["k_protein2dna_score_local", "k_protein2dna_region_local_pack", "k_protein2dna_path",
                                   "k_protein2dna_ckpt_cont_local", "k_protein2dna_path_cont_local"], [128, 256]),
    ("protein2dna", "four-waves"): (["kmw_protein2dna_score_local", "kmw_protein2dna_region_local_pack"], [128, 256, 512, 1024]),
    ("protein2dna", "general"): (["kmw_protein2dna_score", "kmw_protein2dna_region_pack"], [128, 256, 512, 1024]),
    ("protein2dna", "two-slot"): (["kmw_protein2dna_region_local"], [128, 512]),
    ("protein2dna", "cont-masks"): (["k_protein2dna_ckpt_cont", "k_protein2dna_path_cont"], [128, 256]),
    ("ner/dna", "one-wave"): (["k_ner_score_local", "k_ner_region_local_pack", "k_ner_path", "k_ner_ckpt_cont_local",
                               "k_ner_path_cont_local"], [256]),
    ("ner/dna", "four-waves"): (["kmw_ner_score_local", "kmw_ner_region_local_pack"], [256, 1024]),
    ("ner/dna", "general"): (["k_ner_score", "k_ner_region_pack"], [256]),
    ("ner/dna", "two-slot"): (["kmw_ner_region_local"], [256, 1024]),
    ("ner/dna", "cont-masks"): (["k_ner_ckpt_cont", "k_ner_path_cont"], [256]),
}
for _family in ("affine:local/dna", "affine:local/protein"):
    COVERAGE_32.update({
        (_family, "one-wave"): (["k_affine_score_local", "k_affine_region_local_pack", "k_affine_path", "k_affine_ckpt_cont_local",
                                 "k_affine_path_cont_local"], [256]),
        (_family, "four-waves"): (["kmw_affine_score_local", "kmw_affine_region_local_pack"], [256, 1024]),
        (_family, "general"): (["kmw_affine_score", "kmw_affine_region_pack"], [256, 1024]),
        (_family, "two-slot"): (["kmw_affine_region_local"], [256, 1024]),
        (_family, "cont-masks"): (["k_affine_ckpt_cont", "k_affine_path_cont"], [256])})
for _family in ("affine:global/dna", "affine:bestfit/dna", "affine:overlap/dna", "affine:global/protein"):
    COVERAGE_32.update({
        (_family, "one-wave"): (["k_affine_score", "k_affine_region_pack", "k_affine_path", "k_affine_ckpt_cont_local",
                                 "k_affine_path_cont_local"], [256]),
        (_family, "four-waves"): (["kmw_affine_score", "kmw_affine_region_pack"], [256, 1024]),
        (_family, "two-slot"): (["kmw_affine_region"], [256, 1024]),
        (_family, "cont-masks"): (["k_affine_ckpt_cont", "k_affine_path_cont"], [256])})
# the sub-alignments' host and device routes run the continuation kernels of the default choice at those kernels' strips
for (_family, _form), (_names, _bands) in list(COVERAGE_32.items()):
    if _form == "one-wave":
        _cont = [n for n in _names if n.endswith("_cont_local")]
        _at = COVERAGE_32[(_family, "cont-masks")][1]
        COVERAGE_32[(_family, "host-route")] = COVERAGE_32[(_family, "device-route")] = (_cont, _at)


def test_the_coverage_table_lists_every_32_bit_case():
    held = {(family, form) for family in FAMILIES for form in ec.FORMS32 if ec.form32_bands(family, form)}
    assert held == set(COVERAGE_32), (sorted(held - set(COVERAGE_32)), sorted(set(COVERAGE_32) - held))


@pytest.mark.parametrize("family, form", sorted(COVERAGE_32), ids=["%s-%s" % k for k in sorted(COVERAGE_32)])
def test_choose_kernel_names_what_the_32_bit_cases_expect(family, form):
    """For the batch of every band a case runs -- its own query lengths, 256 compute units, the case's switches -- choose_kernel
    names the kernels the coverage table lists, and the band lies on a strip or workgroup edge of one of them."""
    names, rows = COVERAGE_32[(family, form)]
    bands = ec.form32_bands(family, form)
    assert [b[0] for b in bands] == rows
    for band in bands:
        lengths = [len(p["q"]) for p in ec.band_pairs(family, band) if p.get("point", "default") == "default"]
        got = ec.form_launches(family, form, lengths)
        assert [got[w]["name"] for w in ec.FORMS32[form][1]] == names, (band, got)
        assert band[0] in ec.form_boundaries([got[w] for w in ec.FORMS32[form][1]]), (band, got)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_column_band_takes_the_cooperating_waves(family):
    """Every query of the column band has three strips of 64 x 4 rows: under C4GPU_MW=4, and by default where the family has
    the eight-wave form, the score and region passes run on cooperating waves (64-column chunks, the 256-column ring)."""
    lengths = [len(p["q"]) for p in ec.band_pairs(family, ("cols", 530))]
    assert min(lengths) >= 530
    for form in ("four-waves", "eight-waves"):
        if ec.form32_bands(family, form):
            got = ec.form_launches(family, form, lengths)
            assert got["score"]["waves"] == got["region"]["waves"] == (4 if form == "four-waves" else 8), got


@pytest.mark.parametrize("form", sorted(ec.FORMS_SEEDED))
def test_choose_kernel_names_what_the_seeded_column_cases_expect(form):
    """Every seeded and packed form also runs the column band (end cells, target ends and intron ends on c - 1, c, c + 1 for
    c = 64 ... 320; at a dump every 32 columns each c is a dump column): the pairs of it that find_path_batch windows lead to
    the kernels of COVERAGE_SEEDED -- for the six-row and the long form through the one query long enough to select them."""
    family, env, about = ec.FORMS_SEEDED[form]
    pairs = ec.band_pairs(family, ec.seeded_col_band(form))
    lengths = [len(p["q"]) for p in pairs if len(p["t"]) >= (4 << int(env["SEED_KSHIFT"]))]
    assert len(lengths) >= 2 and min(lengths) > 2 * 64 * 3
    got = ec.seeded_geometry(form, lengths, len(set("".join(p["t"] for p in pairs))) if form != "pk16/c8" else 7)
    assert [got[w]["name"] for w in about] == COVERAGE_SEEDED[form][0], got


COVERAGE_SEEDED = {
    "win32/est2genome/nw2": (["kmw8_est2genome_score_local_seed1", "kmw2_est2genome_region_local_pack_seed2"], [128, 192, 384, 1024]),
    "win32/est2genome/nw4": (["kmw8_est2genome_score_local_seed1", "kmw_est2genome_region_local_pack_seed2"], [128, 192, 768, 1024]),
    "win32/est2genome/mw4": (["kmw_est2genome_score_local_seed1"], [256, 1024]),
    "win32/protein2genome": (["kmw8_protein2genome_score_local_seed1", "kmw_protein2genome_region_local_pack_seed2"], [64, 128, 512]),
    "win32/protein2genome/mw4": (["kmw_protein2genome_score_local_seed1"], [128, 512]),
    "pk16/plain": (["kpk16b_est2genome"], [256, 1024]), "pk16/asm": (["kpk16_est2genome"], [256, 1024]),
    "pk16/counters": (["kpk16c_est2genome"], [256, 1024]), "pk16/io0": (["kpk16d_est2genome"], [256, 1024]),
    "pk16/io1": (["kpk16e_est2genome"], [256, 1024]), "pk16/io2": (["kpk16f_est2genome"], [256, 1024]),
    "pk16/nw8": (["kpk16g_est2genome"], [128, 1024]), "pk16/r6": (["kpk16h_est2genome"], [384, 1024, 1536]),
    "pk16/long": (["kpk16j_est2genome"], [384, 1536]), "pk16/c8": (["kpk16i_est2genome"], [256, 1024]),
    "win16/2": (["kwin16_est2genome_r3w3"], [192]), "win16/3": (["kwin16_est2genome_r2w4"], [128]),
    "win16/4": (["kwin16_est2genome_r6w2"], [384]), "win16/5": (["kwin16_est2genome_r4w2n4"], [256, 1024]),
    "win16/6": (["kwin16_est2genome_r2w4n8"], [128, 1024]), "win16/7": (["kwin16_est2genome_r2w4n4"], [128, 512]),
    "win16/8": (["kwin16_est2genome_r4w2n2"], [256, 512]), "win16/9": (["kwin16_est2genome_r4w2"], [256]),
    "win16/10": (["kwin16_est2genome_r4w3n2"], [256, 512]),
    "ck16/2": (["kck16r_est2genome_r4w2"], [256]), "ck16/3": (["kck16r_est2genome_r3w3"], [192]),
    "ck16/4": (["kck16r_est2genome_r2w4"], [128]), "ck16/5": (["kck16r_est2genome_r4w2n4"], [256, 1024]),
    "ck16/6": (["kck16r_est2genome_r4w2n2"], [256, 512]), "ck16/7": (["kck16r_est2genome_r6w2n3"], [384]),
    "ck16/8": (["kck16r_est2genome_r6w2"], [384]), "ck16/9": (["kck16r_est2genome_r4w3n4"], [256, 1024]),
    "ck16/unrooted": (["kck16_est2genome_r4w2"], [256]),
}


@pytest.mark.parametrize("form", sorted(ec.FORMS_SEEDED))
def test_choose_kernel_names_what_the_seeded_cases_expect(form):
    """The same for the windowed region pass and the packed forms: the pairs of each band that find_path_batch windows (targets
    of 4 << kshift columns and more) lead to the kernels of the coverage table."""
    family, env, about = ec.FORMS_SEEDED[form]
    names, rows = COVERAGE_SEEDED[form]
    bands = ec.seeded_bands(form)
    assert [(b[1] if b[0] == "c8" else b)[0] for b in bands] == rows
    for band in bands:
        pairs = ec.band_pairs(family, band)
        codes = len(set("".join(p["t"] for p in pairs)))
        row = (band[1] if band[0] == "c8" else band)[0]
        for k, call in enumerate(ec.seeded_calls(form, band)):
            lengths = [len(pairs[n]["q"]) for n in call
                       if pairs[n].get("point", "default") == "default" and len(pairs[n]["t"]) >= (4 << int(env["SEED_KSHIFT"]))]
            assert len(lengths) >= 2 and min(lengths) > 2 * 64 * 3        # the windows' domain: more than two strips of their kernel
            got = ec.seeded_geometry(form, lengths, codes)
            if k == 1:            # the queries beyond the staged rows: six rows per lane, beyond those the long form (seven codes, barriers: the form that loads per step)
                beyond = ("kpk16d_est2genome" if form in ("pk16/c8", "pk16/io1") else
                          "kpk16j_est2genome" if form == "pk16/r6" else "kpk16h_est2genome")
                assert got["seed1"]["name"] == beyond, (band, got)
                continue
            assert [got[w]["name"] for w in about] == names, (band, got)
            at = ec.form_boundaries([got[w] for w in about])
            assert row in at or (form == "pk16/r6" and row == got["seed1"]["staged_rows"]), (band, at)
