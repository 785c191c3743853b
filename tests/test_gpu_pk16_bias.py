"""The biased staged forms of the packed score pass (exonerate_amd/csrc/c4_viterbi16_kernel.h, BIAS: scores carried as real +
PK16_BIAS, the match states' maxima through v_pk_maximum3_f16) at the smallest shapes where that code can go wrong.  Every pair of
every case is compared bit-exactly (score, region, operations) with the oracle, and the whole call with the same call under
C4GPU_PK16_IO=0 (integer maxima, the form that loads per step); each case asserts from C4GPU_TRACE which kernel ran.

The engine sends a pair to the windowed route -- the only caller of the packed score pass -- when its query has more rows than two
strips of the window kernel (Q >= 384) and its target at least four dump intervals (T >= 16 here); the smaller pairs of the ragged
batch are served by the one-pass kernels in the same call and are held to the oracle like the others.  Every case gives the
packed pass an odd number of jobs, so that its last lane pair repeats a job."""
import random
import re

import pytest

import exonerate_amd as ex
import oracle_lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _mutate(rng, s, rate):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice("ACGT"))
        elif r < 2 * rate / 3:
            out.append(ch + rng.choice("ACGT"))
        elif r >= rate:
            out.append(ch)
    return "".join(out)


def _pair(rng, ql, tl, intron=0):
    """a query of ql rows and a target of tl columns that holds a mutated copy of it (cut to fit), with one GT..AG intron of
    `intron` columns in its middle"""
    q = _rand(rng, ql)
    body = _mutate(rng, q, 0.04)
    if intron and ql > 60:
        h = len(body) // 2
        body = body[:h] + "GT" + _rand(rng, intron - 4) + "AG" + body[h:]
    body = body[:tl]
    left = rng.randrange(0, tl - len(body) + 1)
    return q, _rand(rng, left) + body + _rand(rng, tl - len(body) - left)


def _dicts(alns):
    return [a.as_dict() if a else None for a in alns]


def _check(eng, model, pairs, monkeypatch, capfd, kernel, env=None, dpmemory=0, kshift="2", n_packed=None):
    """find_path on the default (biased) route and with C4GPU_PK16_IO=0; both against the oracle; the kernel and the number of jobs
    the packed pass saw (n_packed; all of them by default) from the trace"""
    monkeypatch.setenv("C4GPU_TRACE", "1")
    monkeypatch.setenv("C4GPU_SEED_KSHIFT", kshift)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    got = _dicts(eng.find_path(model, pairs, dpmemory=dpmemory, threshold=20))
    err = capfd.readouterr().err
    first = [l for l in err.splitlines() if "seeded pass 1 with kernel" in l]
    assert first and all(kernel + "_est2genome" in l for l in first), (kernel, first, err[-800:])
    seen = [int(n) for n in re.findall(r"windowed region pass: (\d+) pairs", err)]
    assert seen == [len(pairs) if n_packed is None else n_packed], (seen, err[-800:])
    want = [oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=dpmemory, threshold=20) for q, t in pairs]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, k
    if kernel != "kpk16d":
        monkeypatch.setenv("C4GPU_PK16_IO", "0")
        plain = _dicts(eng.find_path(model, pairs, dpmemory=dpmemory, threshold=20))
        err = capfd.readouterr().err
        assert "kpk16d_est2genome" in err and kernel + "_est2genome" not in err, err[-800:]
        assert plain == got
        monkeypatch.delenv("C4GPU_PK16_IO")
    return got


def test_ragged_batch_of_nine_jobs(eng, monkeypatch, capfd):
    """Nine jobs on kpk16f, odd on purpose (the last lane pair repeats its job): Q in {384, 385, 700, 1000, 1023} against T in
    {40, 64, 130, 700, 5000}, N in a query and in a target, a true spliced alignment with an intron longer than min_intron and a
    planted GT..AG pair closer than min_intron (the too-short branch adds -32 768 to a high score), a dump every four columns so
    that the windows start from the dumps.  Q = 1 000 leaves rows 1 001 - 1 023 dead, Q = 384 / 385 leave two and a half waves
    of a workgroup without a row.  The engine sends a pair to the windowed route, the packed pass's only caller, when Q + 1
    exceeds two strips of the window kernel (Q >= 384) and T >= 16: Q in {1, 2, 63, 64, 255, 256, 257, 383} and T = 3 cannot reach
    this kernel; such pairs ride in the same call, are served by the one-pass kernels and are held to the oracle all the same."""
    rng = random.Random(20260119)
    model = ex.Model("est2genome")
    # an exon boundary with GT..AG only 12 columns apart (min_intron is 30): 700 rows against 5 000 columns
    qs = _rand(rng, 700)
    short = (qs, (_rand(rng, 100) + qs[:350] + "GT" + _rand(rng, 8) + "AG" + qs[350:] + _rand(rng, 5000))[:5000])
    packed = [_pair(rng, 1000, 5000, intron=300), _pair(rng, 1023, 700), _pair(rng, 700, 5000, intron=90), short,
              _pair(rng, 384, 130), _pair(rng, 385, 64), _pair(rng, 1000, 40), _pair(rng, 700, 64), _pair(rng, 1023, 130)]
    q, t = packed[1]
    packed[1] = (q[:500] + "N" + q[501:], t)
    q, t = packed[2]
    packed[2] = (q, t[:2500] + "NNN" + t[2503:])
    others = [_pair(rng, 383, 130), _pair(rng, 257, 130), _pair(rng, 256, 64), _pair(rng, 255, 40), _pair(rng, 64, 700),
              _pair(rng, 63, 130), _pair(rng, 2, 40), _pair(rng, 1, 3)]
    pairs = packed[:5] + others[:4] + packed[5:] + others[4:]
    got = _check(eng, model, pairs, monkeypatch, capfd, "kpk16f", {"C4GPU_PK16_NW8": "0"}, n_packed=9)
    assert sum(1 for g in got if g) >= 8


@pytest.mark.parametrize("kernel, env, sizes, alpha", [
    ("kpk16g", {}, [(600, 900), (420, 500), (513, 700)], "ACGT"),
    ("kpk16e", {"C4GPU_PK16_IO": "1", "C4GPU_PK16_NW8": "0"}, [(600, 900), (420, 500), (513, 700)], "ACGT"),
    ("kpk16i", {"C4GPU_PK16_NW8": "0"}, [(600, 900), (420, 500), (513, 700)], "ACGTNRY"),
    ("kpk16h", {}, [(1030, 400), (700, 300), (1100, 500)], "ACGT"),
    ("kpk16j", {}, [(1600, 300), (700, 300), (1540, 400)], "ACGT"),
])
def test_other_staged_kernels(eng, monkeypatch, capfd, kernel, env, sizes, alpha):
    rng = random.Random(len(kernel) * 1000 + sizes[0][0])
    model = ex.Model("est2genome")
    pairs = [_pair(rng, ql, tl, intron=60 if tl > ql + 100 else 0) for ql, tl in sizes]
    if len(alpha) > 4:                               # seven residue codes in the targets
        q, t = pairs[0]
        pairs[0] = (q, t[:50] + "NRY" + t[53:])
    monkeypatch.setenv("C4GPU_TRACE", "1")
    monkeypatch.setenv("C4GPU_SEED_KSHIFT", "2")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    got = _dicts(eng.find_path(model, pairs, dpmemory=0, threshold=20))
    err = capfd.readouterr().err
    first = [l for l in err.splitlines() if "seeded pass 1 with kernel" in l]
    assert first and all(kernel + "_est2genome" in l for l in first), (first, err[-800:])
    for k, (q, t) in enumerate(pairs):
        assert got[k] == oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=0, threshold=20), k
    monkeypatch.setenv("C4GPU_PK16_IO", "0")
    assert got == _dicts(eng.find_path(model, pairs, dpmemory=0, threshold=20))
    assert "kpk16d_est2genome" in capfd.readouterr().err


def test_top_of_the_range(eng, monkeypatch, capfd):
    """A match score of 15 and a perfect-match pair of 1 023 rows: the real score is 15 345, (Q + 1) x 15 = 15 360 <= 16 000, the
    biased halves reach PK16_BIAS + 15 345, just under the largest finite half."""
    params = ex.default_params()
    for i in range(24):
        for j in range(24):
            if params.dna_submat[i][j] == 5:
                params.dna_submat[i][j] = 15
    model = ex.Model("est2genome", params=params)
    rng = random.Random(15)
    q = _rand(rng, 1023)
    pairs = [(q, _rand(rng, 40) + q + _rand(rng, 37)), _pair(rng, 600, 800), _pair(rng, 1023, 300)]
    got = _check(eng, model, pairs, monkeypatch, capfd, "kpk16f", {"C4GPU_PK16_NW8": "0"})
    assert got[0]["score"] == 15345


def test_guard_fallback(eng, monkeypatch, capfd):
    """A gap-open penalty inside the band the biased form cannot carry (past PK16_ADDEND_MAX, far from -32 768) but inside the
    packed pass's own guard (16 000): the per-step form with integer maxima serves, and the results are the oracle's."""
    params = ex.default_params()
    params.gap_open = -9000
    model = ex.Model("est2genome", params=params)
    rng = random.Random(9000)
    pairs = [_pair(rng, 600, 900, intron=80), _pair(rng, 1000, 700), _pair(rng, 513, 2000, intron=200)]
    _check(eng, model, pairs, monkeypatch, capfd, "kpk16d")


def test_guard_fallback_by_a_site_sum(eng, monkeypatch, capfd):
    """The engine's own worst site sum (Engine::init_host: every PSSM row at its smallest entry, the pre-splice constant folded in):
    eight rows of -1 000 in the forward 5' model make a site's worst sum -8 000 and below, past PK16_ADDEND_MAX; -900 per row keeps
    it inside (-7 200 - 30 and the model's other rows).  Outside: the per-step form; inside: the biased form; both the oracle's."""
    rng = random.Random(8000)
    pairs = [_pair(rng, 600, 900, intron=80), _pair(rng, 1000, 700), _pair(rng, 513, 2000, intron=200)]
    for per_row, kernel in ((-1000, "kpk16d"), (-900, "kpk16f")):
        params = ex.default_params()
        sp = params.splice[0]
        assert sp.model_length >= 8
        for r in range(8):
            for c in range(5):
                sp.data[r][c] = per_row
        worst = sum(min(0.0, min(sp.data[r][c] for c in range(5))) for r in range(sp.model_length))
        assert (worst - 32 < -7296) == (kernel == "kpk16d"), worst          # (the constant -30, rounding and one of slack)
        model = ex.Model("est2genome", params=params)
        _check(eng, model, pairs, monkeypatch, capfd, kernel, {"C4GPU_PK16_NW8": "0"})
