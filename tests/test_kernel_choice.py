"""The kernel each launch gets (exonerate_amd/csrc/c4_kernel_choice.h: choose_kernel, choose_ck16_rooted_shape, pk16_enabled), on
the host: tests/kernel_choice_sim.hip links the product's choice against the real kernel table of libc4gpu.so.  One row per
launch shape and the kernel it must get, at the edges of every condition the choice reads.  The device has 256 compute units."""
import pytest

import kernel_choice_sim_lib as kc
from kernel_choice_sim_lib import SCORE, PATH, REGION, CKPT

E2G = kc.FAMILY["est2genome"]
CU = 256
F16, SS, ST = "fmt16", "needs_ss16", "staged_codes"


def score_pass(qlen, n, switches=None, **facts):
    """The score pass with dumps of the windowed region pass: est2genome, local, `n` jobs of query length `qlen` (or a list of
    lengths) that all fit the packed pass, five residue codes, a dump every 4 096 columns."""
    f = dict(family=E2G, mode=SCORE, local=1, local_exact=1, seed_mode=1, kshift=12, pk16_params_ok=1, pk16_all_fit=1, tdense_n=5,
             cu_count=CU)
    f.update(facts)
    return kc.choose(qlen if isinstance(qlen, list) else (qlen, n), switches, **f)


def windows(qlens, switches=None, **facts):
    f = dict(family=E2G, mode=REGION, local=1, local_exact=1, starts_pack=1, seed_mode=2, kshift=12, fmt16=1, pk16_params_ok=1,
             tdense_n=5, ss16_built=1, cu_count=CU)
    f.update(facts)
    return kc.choose(qlens, switches, **f)


def plain(mode, qlens, switches=None, **facts):
    f = dict(family=E2G, mode=mode, local=1, local_exact=1, cu_count=CU)
    f.update(facts)
    return kc.choose(qlens, switches, **f)


STAGED = {F16, SS, ST}


@pytest.mark.parametrize("n, switches, kernel", [
    (2, {}, "kpk16g"), (511, {}, "kpk16g"), (512, {}, "kpk16g"),       # (n + 1) / 2 <= 256 compute units
    (513, {}, "kpk16f"), (4096, {}, "kpk16f"),
    (512, {"PK16_NW8": 0}, "kpk16f"), (4096, {"PK16_NW8": 1}, "kpk16g"), (4096, {"PK16_NW8": 2}, "kpk16f"),
    (512, {"PK16_IO": 1}, "kpk16e"),                                   # the eight-wave form has progress counters only
])
@pytest.mark.parametrize("codes", [1, 4, 5, 6])
def test_staged_score_pass_by_job_count(n, switches, kernel, codes):
    for q in (300, 1023):                                                  # Q + 1 <= 1 024
        assert score_pass(q, n, switches, tdense_n=codes) == (kernel + "_est2genome", STAGED)


@pytest.mark.parametrize("q, switches, kernel, flags", [
    (1023, {}, "kpk16f", STAGED),
    (1024, {}, "kpk16h", STAGED), (1535, {}, "kpk16h", STAGED),           # Q + 1 = 1 025, 1 536
    (1024, {"PK16_R6": 0}, "kpk16d", {F16, SS}), (1535, {"PK16_R6": 0}, "kpk16d", {F16, SS}),
    (1024, {"PK16_IO": 1}, "kpk16d", {F16, SS}),
    (1536, {}, "kpk16j", STAGED), (3100, {}, "kpk16j", STAGED),           # Q + 1 = 1 537
    (1536, {"PK16_LONG": 0}, "kpk16d", {F16, SS}), (1536, {"PK16_R6": 0}, "kpk16d", {F16, SS}),
    (31999, {}, "kpk16j", STAGED),                                          # 16-bit dump rows: Q < 32 000
    (32000, {}, "kpk16b", {SS}),
])
def test_score_pass_by_query_rows(q, switches, kernel, flags):
    for n in (2, 4096):            # the eight-wave form is for queries of one workgroup's strips alone
        expect = ("kpk16g" if kernel == "kpk16f" and n == 2 else kernel) + "_est2genome"
        assert score_pass(q, n, switches) == (expect, flags)
        # one long query among short ones decides
        assert score_pass([q] + [200] * (n - 1), n, switches) == score_pass([200] * (n - 1) + [q], n, switches) == (expect, flags)


@pytest.mark.parametrize("codes, q, switches, kernel, flags", [
    (6, 1023, {}, "kpk16f", STAGED),
    (7, 1023, {}, "kpk16i", STAGED), (8, 1023, {}, "kpk16i", STAGED), (8, 300, {}, "kpk16i", STAGED),
    (9, 1023, {}, "kpk16d", {F16, SS}),
    (7, 1023, {"PK16_C8": 0}, "kpk16d", {F16, SS}), (8, 1023, {"PK16_C8": 0}, "kpk16d", {F16, SS}),
    (7, 1023, {"PK16_IO": 1}, "kpk16d", {F16, SS}), (8, 1023, {"PK16_IO": 1}, "kpk16d", {F16, SS}),
    (7, 1023, {"PK16_IO": 0}, "kpk16d", {F16, SS}),
    (7, 1024, {}, "kpk16d", {F16, SS}), (8, 1536, {}, "kpk16d", {F16, SS}),          # no eight-code form beyond 1 024 rows
    (0, 1023, {}, "kpk16b", {SS}), (0, 300, {}, "kpk16b", {SS}),                     # no dense code table: 32-bit dumps
])
def test_score_pass_by_residue_codes(codes, q, switches, kernel, flags):
    for n in (2, 512, 4096):       # (seven and eight codes never take the eight-wave form)
        expect = "kpk16g" if kernel == "kpk16f" and n <= 512 else kernel
        assert score_pass(q, n, switches, tdense_n=codes) == (expect + "_est2genome", flags)


@pytest.mark.parametrize("switches, facts, kernel, flags", [
    ({"PK16_IO": 1}, {}, "kpk16e", STAGED), ({"PK16_IO": 0}, {}, "kpk16d", {F16, SS}), ({"PK16_IO": 3}, {}, "kpk16e", STAGED),
    ({"WIN16": 0}, {}, "kpk16b", {SS}), ({"WIN16": 5}, {}, "kpk16f", STAGED),
    ({}, {"kshift": 16}, "kpk16b", {SS}), ({}, {"kshift": 15}, "kpk16f", STAGED),
    ({"PK16": 3}, {}, "kpk16", set()), ({"PK16": 4}, {}, "kpk16c", {SS}),
    ({"PK16": 2}, {}, "kpk16b", {SS}), ({"PK16": 5}, {}, "kpk16b", {SS}),           # only PK16=1 exactly takes the 16-bit dumps
    ({"PK16": 3, "WIN16": 0}, {}, "kpk16", set()),
])
def test_score_pass_switches_and_guards(switches, facts, kernel, flags):
    assert score_pass(1000, 4096, switches, **facts) == (kernel + "_est2genome", flags)


@pytest.mark.parametrize("n, switches, facts", [
    (4096, {"PK16": 0}, {}), (1, {}, {}), (4096, {}, {"pk16_all_fit": 0}), (4096, {}, {"pk16_params_ok": 0}),
    (256, {"PK16": 0}, {}), (257, {"PK16": 0}, {}), (256, {"PK16": 0, "MW": 4}, {}), (1, {"MW": 4}, {}),
    (256, {"PK16": 0, "MW": 0}, {}),
])
def test_seeded_score_pass_in_32_bits(n, switches, facts):
    # eight waves while 8 n <= 8 x 256 compute units, four above that or with C4GPU_MW=4 (C4GPU_MW=0 means nothing here)
    eight = n <= 256 and switches.get("MW") != 4
    assert score_pass(1000, n, switches, **facts) == ("kmw8_est2genome_score_local_seed1" if eight else "kmw_est2genome_score_local_seed1", set())


def test_seeded_score_pass_of_another_family():
    assert score_pass(1000, 4096, family=kc.FAMILY["protein2genome"]) == ("kmw_protein2genome_score_local_seed1", set())
    assert score_pass(1000, 256, family=kc.FAMILY["protein2genome"]) == ("kmw8_protein2genome_score_local_seed1", set())


WIN16_SHAPES = ["r4w2", "r3w3", "r2w4", "r6w2", "r4w2n4", "r2w4n8", "r2w4n4", "r4w2n2", "r4w2", "r4w3n2"]


@pytest.mark.parametrize("qlens, shape", [
    ((255, 512), 0), ((255, 513), 0),                      # one strip of 256 rows per job
    ((256, 512), 4), ((256, 2), 4), ((256, 511), 4),       # two and more: four waves while (n + 1) / 2 <= 256 compute units
    ((256, 513), 7), ((3000, 4096), 7),                    # ... two above that
    ([512] * 300 + [200] * 300, 7), ([512] * 299 + [511] + [200] * 300, 0),      # strips = 2 n, 2 n - 1
    ([512] * 200 + [200] * 200, 4), ([512] * 199 + [511] + [200] * 200, 0),
])
@pytest.mark.parametrize("win16", [None, 1, 0, -1])
def test_packed_windows_by_the_jobs(qlens, shape, win16):
    switches = {} if win16 is None else {"WIN16": win16}
    assert windows(qlens, switches) == ("kwin16_est2genome_" + WIN16_SHAPES[shape], {F16})


@pytest.mark.parametrize("win16", range(2, 12))
def test_packed_windows_pinned_shape(win16):
    shape = 0 if win16 in (9, 11) else win16 - 1            # 9: the default shape; beyond the last shape: the default shape
    for qlens in ((255, 512), (256, 512), (256, 4096)):
        assert windows(qlens, {"WIN16": win16}) == ("kwin16_est2genome_" + WIN16_SHAPES[shape], {F16})


def test_windows_in_32_bits():
    for qlens in ((255, 512), (256, 4096)):
        assert windows(qlens, fmt16=0) == ("kmw2_est2genome_region_local_pack_seed2", set())
        assert windows(qlens, {"WIN_NW": 4}, fmt16=0) == ("kmw_est2genome_region_local_pack_seed2", set())
        assert windows(qlens, {"WIN_NW": 3}, fmt16=0) == ("kmw_est2genome_region_local_pack_seed2", set())
        assert windows(qlens, {"WIN_NW": 2, "MW": 4}, fmt16=0) == ("kmw2_est2genome_region_local_pack_seed2", set())
    # a family without the two-wave form keeps four
    assert windows((300, 512), fmt16=0, family=kc.FAMILY["protein2genome"]) == ("kmw_protein2genome_region_local_pack_seed2", set())


@pytest.mark.parametrize("mode, stem", [(SCORE, "score_local"), (REGION, "region_local_pack")])
def test_plain_passes_by_strips(mode, stem):
    facts = {"starts_pack": 1} if mode == REGION else {}
    one, four, eight = ("%s_est2genome_%s" % (k, stem) for k in ("k", "kmw", "kmw8"))
    # strips of 64 x 4 rows: four waves from three strips per job, eight while 8 n <= 8 x 256 compute units
    assert plain(mode, (511, 300), **facts) == (one, set())
    assert plain(mode, (512, 300), **facts) == (four, set())
    assert plain(mode, (512, 256), **facts) == (eight, set())
    assert plain(mode, (512, 257), **facts) == (four, set())
    assert plain(mode, (511, 256), **facts) == (one, set())
    assert plain(mode, [1279] * 100 + [200] * 100, **facts) == (eight, set())           # strips = 3 n
    assert plain(mode, [1279] * 99 + [1023] + [200] * 100, **facts) == (one, set())      # 3 n - 1
    assert plain(mode, (512, 256), {"MW": 4}, **facts) == (four, set())
    assert plain(mode, (512, 256), {"MW": 0}, **facts) == (one, set())
    assert plain(mode, (512, 300), {"MW": 0}, **facts) == (one, set())
    assert plain(mode, (512, 300), {"MW": 2}, **facts) == (four, set())
    # blocked launches: the _sub kernels, never on eight waves, C4GPU_WPE read as 0
    for wpe in ({}, {"WPE": 2}):
        assert plain(mode, (511, 256), wpe, blocked=1, **facts) == (one + "_sub", set())
        assert plain(mode, (512, 256), wpe, blocked=1, **facts) == (four + "_sub", set())
        assert plain(mode, (512, 256), dict(wpe, MW=0), blocked=1, **facts) == (one + "_sub", set())


def test_plain_passes_scope_and_pack():
    # parameters outside the local shortcut's range, or a model that is not local: every mask kept, no cooperating-wave form
    for facts in ({"local_exact": 0}, {"local": 0}):
        assert plain(SCORE, (512, 300), **facts) == ("k_est2genome_score", set())
        assert plain(REGION, (512, 300), starts_pack=1, **facts) == ("k_est2genome_region_pack", set())
    # region starts in two slots: C4GPU_PACK=0, or a job whose start does not fit 31 bits
    assert plain(REGION, (512, 300), {"PACK": 0}, starts_pack=1) == ("kmw_est2genome_region_local", set())
    assert plain(REGION, (512, 300), starts_pack=0) == ("kmw_est2genome_region_local", set())
    assert plain(REGION, (512, 256), starts_pack=0) == ("kmw8_est2genome_region_local", set())
    # (two rows per lane in that form: strips of 128 rows, three of them from 257 rows)
    assert plain(REGION, (256, 300), starts_pack=0) == ("kmw_est2genome_region_local", set())
    assert plain(REGION, (255, 300), starts_pack=0) == ("k_est2genome_region_local", set())
    assert plain(PATH, (512, 300)) == ("k_est2genome_path", set())
    assert plain(PATH, (512, 300), blocked=1) == ("k_est2genome_path_sub", set())


@pytest.mark.parametrize("mode, stem", [(PATH, "path"), (CKPT, "ckpt")])
def test_continuation_kernels(mode, stem):
    # the kernels without the row-0 mask where they stay exact; no cooperating-wave form, whatever the sizes
    for qlens in ((10, 5), (3000, 300000)):
        assert plain(mode, qlens, cont=1, cont_free=1) == ("k_est2genome_%s_cont_local" % stem, set())
        assert plain(mode, qlens, cont=1, cont_free=0) == ("k_est2genome_%s_cont" % stem, set())
        assert plain(mode, qlens, cont=1, cont_free=0, blocked=1) == ("k_est2genome_%s_cont_sub" % stem, set())
        assert plain(mode, qlens, cont=1, cont_free=1, local=0, local_exact=0) == ("k_est2genome_%s_cont_local" % stem, set())


@pytest.mark.parametrize("strips, n, rows_max, shape", [
    (199, 100, 300, "r6w2"), (200, 100, 300, "r4w2n2"), (299, 100, 900, "r4w2n2"), (300, 100, 900, "r4w3n4"),      # 2 n, 3 n
    (1, 1, 200, "r6w2"), (2, 1, 300, "r4w2n2"), (3, 1, 600, "r4w3n4"),
    (400, 100, 1024, "r4w3n4"), (400, 100, 1025, "r6w2n3"), (500, 100, 1152, "r6w2n3"), (500, 100, 1153, "r4w3n4"),
    (399, 100, 1100, "r4w3n4"), (299, 100, 1100, "r4w2n2"), (199, 100, 1100, "r6w2"),                              # ... from 4 n strips
])
def test_rooted_checkpoint_shape_by_the_jobs(strips, n, rows_max, shape):
    assert kc.ck16_rooted(strips, n, rows_max) == "kck16r_est2genome_" + shape
    assert kc.ck16_rooted(strips, n, rows_max, {"CK16": 1, "CK16_ROOT": 1}) == "kck16r_est2genome_" + shape


@pytest.mark.parametrize("ck16, shape", [(2, "r4w2"), (3, "r3w3"), (4, "r2w4"), (5, "r4w2n4"), (6, "r4w2n2"), (7, "r6w2n3"),
                                         (8, "r6w2"), (9, "r4w3n4"), (10, "r6w2")])
def test_rooted_checkpoint_pinned_shape(ck16, shape):
    for strips, n, rows_max in ((199, 100, 300), (300, 100, 900), (500, 100, 1100)):
        assert kc.ck16_rooted(strips, n, rows_max, {"CK16": ck16}) == "kck16r_est2genome_" + shape


def test_the_three_errors():
    assert plain(CKPT, (512, 300)) == ("error", "no compiled kernel for this model/mode")
    assert plain(SCORE, (512, 300), span=1) == ("error", "no compiled kernel for this model/mode")
    assert score_pass(1000, 4096, local_exact=0) == ("error", "no seeded kernel for this launch")
    assert score_pass(1000, 4096, family=kc.FAMILY["affine"], mode=REGION, starts_pack=1) == ("error", "no seeded kernel for this launch")
    assert windows((300, 512), starts_pack=0) == ("error", "no seeded kernel for this launch")
    assert windows((300, 512), {"PACK": 0}) == ("error", "no seeded kernel for this launch")
    assert windows((300, 512), ss16_built=0) == ("error", "no packed window kernel for this launch")
    assert windows((300, 512), fmt16=0, ss16_built=0)[0] == "kmw2_est2genome_region_local_pack_seed2"


def test_packed_score_pass_enabled():
    """One wording for the engine's launch, the stage (does it build the packed splice array) and find_path_batch (the dump
    interval): est2genome, parameters inside 16 bits, two jobs or more, C4GPU_PK16 not 0."""
    assert kc.pk16_enabled("est2genome", True, 2) and kc.pk16_enabled("est2genome", True, 4096)
    assert not kc.pk16_enabled("est2genome", True, 1)
    assert not kc.pk16_enabled("est2genome", False, 4096)
    assert not kc.pk16_enabled("est2genome", True, 4096, {"PK16": 0})
    for pk in (1, 2, 3, 4, 7):
        assert kc.pk16_enabled("est2genome", True, 4096, {"PK16": pk})
    for family in ("affine", "protein2dna", "protein2genome"):
        assert not kc.pk16_enabled(family, True, 4096)
