"""The seeded annotated cases of annot_cases.py, oracle only: in every family the annotation decides at least a third of the jobs
or pairs, and the variants that annotate nothing change nothing -- so that the device tests built on them (test_gpu_annotation.py)
cannot pass on inputs the veto never touches."""
import pytest

import exonerate_amd as ex
import annot_cases as ac


@pytest.mark.parametrize("index", range(len(ac.DERIVED_MODELS)))
def test_annotation_decides_the_derived_model_jobs(index):
    q, t, jobs = ac.derived_case()
    assert 280 <= len(jobs) <= 320 and all(j["region"][2] <= 49 and j["region"][3] <= 49 for j in jobs)
    plain, annot = ac.derived_oracle(index, False), ac.derived_oracle(index, True)
    kinds = [ac.derived_kind(j) for j in jobs]
    assert all(kinds.count(k) >= len(jobs) // 4 for k in (0, 1, 2))
    differ = 0
    for k, p, a in zip(kinds, plain, annot):
        if k == 1:
            assert p == a                     # a rectangle outside the CDS
        else:
            differ += p != a
    assert 3 * differ >= len(jobs), (ac.DERIVED_MODELS[index], differ)


@pytest.mark.parametrize("name", [m[0] for m in ac.LONG_MODELS])
def test_annotation_decides_the_long_queries(name):
    model, q, t = ac.long_case(name)
    plain = ac.long_oracle(name, None, 32)
    assert plain is not None and plain["region"][2] > 128          # the alignment crosses strip boundaries
    differ, may = 0, 0
    for cds, changes in ac.long_cds_variants(len(q)):
        got = ac.long_oracle(name, cds, 32)
        if changes:
            may += 1
            differ += got != plain
        else:
            assert got == plain, cds
    assert 3 * differ >= may, (name, differ, may)


def test_annotation_decides_the_region_and_swap_pairs():
    model = ex.Model("est2genome")
    cases = ac.region_cases()
    assert 3 <= len(cases) <= 4
    differ = 0
    for q, t, cds, region in cases:
        lo, hi = region[0], region[0] + region[2]
        assert (lo > cds[0] and lo < cds[0] + cds[1]) or (hi > cds[0] and hi < cds[0] + cds[1])     # the region cuts the CDS
        differ += ac.oracle_path(model, q, t, cds, region=region) != ac.oracle_path(model, q, t, None, region=region)
    assert 3 * differ >= len(cases)
    for seed in (5151, 5152, 5153):
        pairs = ac.est_pairs(seed, 6)
        differ = sum(ac.oracle_path(model, q, t, cds) != ac.oracle_path(model, q, t, None) for q, t, cds in pairs)
        assert 3 * differ >= len(pairs), seed
