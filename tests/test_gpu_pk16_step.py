"""The step of the staged packed score pass (exonerate_amd/csrc/c4_viterbi16_kernel.h, IO 1 with BIAS): the end-cell test with
best_pk as an operand of the maximum, and the 3'-site length veto as a sign-bit addend.  Small ragged batches through kpk16f (four cooperating waves, four rows per lane: queries of
2 * 64 * 4 + 1 .. 1 023 rows) against targets of 4 << 12 columns -- the shortest the windowed route, the packed pass's only
caller, takes at its default dump distance -- compared bit-exactly (score, region, operations) with oracle_lib.find_path; the
same batches again on kpk16g, which the engine prefers for so few pairs (two rows per lane, eight waves: the same header).

What each pair is there for:
  * `last_cell`: a perfect copy of a 1 023-row query at the very end of the target -- the best end cell is the last row's last
    column (lane 63 of the last wave, the last step of the rectangle);
  * `short`: 513 rows, the other job of `last_cell`'s lanes: every lane from row 516 on holds no row of it, so its half of best_pk
    is the no-row value (0x7BFF) for two and a half waves;
  * `ties`: the query is u + v, 300 rows each; the target starts with v and ends with u, so that neither alignment can grow (an
    est2genome alignment that may grow does, through chance exons): two end cells of 1 500 in rows 600 and 300, in two waves and
    16 000 columns apart (the order of strip_end / reduce_best and of the merge over the waves: the first column wins);
  * `ties_row`: the whole query twice in the target: two end cells of the same score in the last row (the strict < of the
    bookkeeping inside a lane: the first column stays);
  * `introns_fwd`: four exons with planted introns of min_intron - 1, min_intron and min_intron + 1 columns between them, GT..AG
    (the forward strand's intron state): the veto at its edge -- the oracle takes the shortest one as an intron of min_intron
    columns that eats a base of an exon, next to the vetoed candidates of min_intron - 1;
  * `introns_rev`: the same as CT..AC (the reverse strand's intron state; an alignment keeps to one of the two).
The second batch has an odd number of jobs (the last lane pair repeats its job).
The second parameter set gives the two post-splice sites (3' forward, 5' reverse) a best score of 125, just under
PK16_POST_GAIN_MAX = 127 (the golden sets' altparams leave the splice models alone: none qualifies), with an intron penalty that
keeps an intron's net gain where the packed guard wants it: a vetoed candidate then is legitimate + 125 - 32 768.

The oracle's alignments are computed once per parameter set (about 2 s per pair on one core) and shared; every input must have
one, so that no comparison is None == None."""
import functools
import random
import re

import pytest

import exonerate_amd as ex
import oracle_lib

T_COLS = 4 << 12
POST_BEST = 125               # what Engine's guard computes for the raised sites: floor(best sum + 0.5) + 1
NAMES = {"default": ("last_cell", "short", "ties", "ties_row", "introns_fwd", "introns_rev"),
         "high_post_site": ("introns_fwd", "introns_rev", "short")}


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _spliced(rng, exons, min_intron, ends):
    """the four exons in order, between them introns of min_intron - 1, min_intron, min_intron + 1 columns"""
    out = [exons[0]]
    for k, n in enumerate((min_intron - 1, min_intron, min_intron + 1)):
        out.append(ends[0] + _rand(rng, n - 4) + ends[1])
        out.append(exons[k + 1])
    return "".join(out)


def _place(rng, body, left):
    return _rand(rng, left) + body + _rand(rng, T_COLS - left - len(body))


@functools.lru_cache(maxsize=None)
def _inputs(min_intron):
    rng = random.Random(20261021 + min_intron)
    pairs = {}
    q = _rand(rng, 1023)
    pairs["last_cell"] = (q, _rand(rng, T_COLS - 1023) + q)
    q = _rand(rng, 513)
    pairs["short"] = (q, _place(rng, q[:250] + "A" + q[250:], 9000))
    u, v = _rand(rng, 300), _rand(rng, 300)
    pairs["ties"] = (u + v, v + _rand(rng, T_COLS - 600) + u)
    q = _rand(rng, 550)
    pairs["ties_row"] = (q, _place(rng, q + _rand(rng, 3000) + q, 5000))
    for name, lens, ends in (("introns_fwd", (150, 140, 160, 150), ("GT", "AG")), ("introns_rev", (130, 170, 120, 140), ("CT", "AC"))):
        exons = [_rand(rng, n) for n in lens]
        pairs[name] = ("".join(exons), _place(rng, _spliced(rng, exons, min_intron, ends), 1000 + 2000 * len(pairs)))
    assert all(513 <= len(q) <= 1023 and len(t) == T_COLS for q, t in pairs.values())
    return pairs


def _params(which):
    params = ex.default_params()
    if which == "high_post_site":
        # splice[1]: the forward 3' site, splice[3]: the reverse 5' site -- the two a post-splice transition adds.  The row where the
        # consensus stands out most gets its best entry raised until the rows' best entries sum to POST_BEST - 1.4
        for k in (1, 3):
            sp = params.splice[k]
            rows = [[sp.data[r][c] for c in range(5)] for r in range(sp.model_length)]
            best = sum(max(0.0, max(row)) for row in rows)
            r = max(range(len(rows)), key=lambda x: max(rows[x]) - sorted(rows[x])[-2])
            c = rows[r].index(max(rows[r]))
            sp.data[r][c] += (POST_BEST - 1.4) - best
        params.intron_open_penalty = -30 - (POST_BEST - 16)
    return params


@functools.lru_cache(maxsize=None)
def _expected(which):
    params = _params(which)
    model = ex.Model("est2genome", params=params)
    pairs = _inputs(params.min_intron)
    return {n: oracle_lib.find_path(model.c, model.params, pairs[n][0].encode(), pairs[n][1].encode(), dpmemory=0, threshold=20)
            for n in NAMES[which]}


@pytest.mark.parametrize("which", ["default", "high_post_site"])
def test_the_oracle_alone_yields_every_alignment(which):
    """(no GPU) every input has an alignment, and it is the one the input was built for"""
    want = _expected(which)
    params = _params(which)
    pairs = _inputs(params.min_intron)
    assert all(want[n] is not None for n in NAMES[which])
    if which == "high_post_site":
        for k in (1, 3):
            sp = params.splice[k]
            best = sum(max(0.0, max(sp.data[r][c] for c in range(5))) for r in range(sp.model_length))
            assert int(best + 0.5) + 1 == POST_BEST <= 127
    if which == "default":
        assert want["last_cell"]["region"] == [0, T_COLS - 1023, 1023, 1023] and want["last_cell"]["score"] == 5 * 1023
        assert want["ties"]["score"] == 1500 and want["ties"]["region"] == [300, 0, 300, 300]
        assert want["ties_row"]["score"] == 5 * 550 and want["ties_row"]["region"] == [0, 5000, 550, 550]
    m = params.min_intron
    for n, (a, b) in (("introns_fwd", ("5", "3")), ("introns_rev", ("3", "5"))):
        v = want[n]["vulgar"] + " "
        assert want[n]["region"][2] == len(pairs[n][0]), v                    # one alignment over all four exons
        assert len(re.findall(r" %s 0 2 I 0 \d+ %s 0 2 " % (a, b), v)) == 3 == v.count(" I "), v
        for length in (m, m + 1):
            assert " %s 0 2 I 0 %d %s 0 2 " % (a, length - 4, b) in v, (length, v)
        assert " I 0 %d " % (m - 5) not in v, v                               # min_intron - 1 columns: never an intron


def _dicts(alns):
    return [a.as_dict() if a else None for a in alns]


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["default", "high_post_site"])
def test_step_against_the_oracle(eng, monkeypatch, capfd, which):
    params = _params(which)
    model = ex.Model("est2genome", params=params)
    pairs = [_inputs(params.min_intron)[n] for n in NAMES[which]]
    want = [_expected(which)[n] for n in NAMES[which]]
    assert all(w is not None for w in want)
    monkeypatch.setenv("C4GPU_TRACE", "1")
    for kernel, env in (("kpk16f", {"C4GPU_PK16_NW8": "0"}), ("kpk16g", {})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        capfd.readouterr()
        got = _dicts(eng.find_path(model, pairs, dpmemory=0, threshold=20))
        err = capfd.readouterr().err
        first = [l for l in err.splitlines() if "seeded pass 1 with kernel" in l]
        assert first and all(kernel + "_est2genome" in l for l in first), (kernel, first, err[-800:])
        assert [int(n) for n in re.findall(r"windowed region pass: (\d+) pairs", err)] == [len(pairs)], err[-800:]
        for name, g, w in zip(NAMES[which], got, want):
            assert g == w, (kernel, name)
        for k in env:
            monkeypatch.delenv(k)
