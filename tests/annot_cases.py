"""Seeded inputs with CDS annotations (exonerate's --annotation, match.c:276-281: no 1:1 DNA match inside the query's CDS) and
their oracle results, shared by the CPU test that shows the annotation decides them (test_annot_cases.py) and by the device
tests (test_gpu_annotation.py).  Data and plumbing only; the checker is oracle/c4_oracle.c under oracle_set_annotation, itself
pinned on the reference's annotated records (test_oracle_golden.py, test_ner_model.py).

Shapes are the smallest that still reach the code: BSDP-sized rectangles for the derived models, queries just past two strips of
64 x R query rows for the checkpoint route, one of three strips for the cooperating-wave kernels, ~150 x 600 pairs elsewhere.
"""
import contextlib
import functools
import random

import exonerate_amd as ex
from exonerate_amd import _abi
import oracle_lib


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _mutate(rng, s, rate, alpha="ACGT"):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alpha))
        elif r < 2 * rate / 3:
            out.append(ch + rng.choice(alpha))
        elif r >= rate:
            out.append(ch)
    return "".join(out)


@contextlib.contextmanager
def oracle_annotation(cds):
    """The oracle's calls inside the block align a query with this CDS (None: no annotation); always taken away again."""
    oracle_lib.set_annotation(cds)
    try:
        yield
    finally:
        oracle_lib.set_annotation(None)


def oracle_job(model, mode, q, t, region, continuation=None, checkpoints=0):
    """One Viterbi_DP_Func-level call of the oracle as a dict: score, query_start, target_start, query_end, target_end, ops and what the
    checkpoint pass reports: last_srp, the cell size, the first and the last slot of the final cell)."""
    olib = oracle_lib.load()
    vo = oracle_lib.ViterbiOut()
    olib.oracle_viterbi(model.c, model.params, mode, q.encode(), len(q), t.encode(), len(t), _abi.Region(*region),
                        continuation, checkpoints, vo)
    out = {"score": vo.score, "query_start": vo.query_start, "target_start": vo.target_start, "query_end": vo.query_end,
           "target_end": vo.target_end, "ops": [vo.ops[x] for x in range(vo.n_ops)], "last_srp": vo.last_srp,
           "cell_size": vo.cell_size,
           "final_cell": [vo.final_cell[0], vo.final_cell[max(0, vo.cell_size - 1)]]}
    olib.oracle_viterbi_out_clear(vo)
    return out


# ---- derived models (BSDP's terminal and join sub-DPs): one pair, ~300 rectangles of at most 49 x 49 cells -----------------
# (model type, (src state, dst state, start scope, end scope)): those of test_thousands_of_bsdp_sized_jobs_on_derived_models.
# Model.derived("ner", ...) builds a table on the host, but the device has no derived ner family (model_family): none here.
DERIVED_MODELS = [("affine:local", (2, 2, 4, 4)), ("affine:local", (0, 2, 0, 4)), ("est2genome", (2, 2, 4, 4)),
                  ("est2genome", (5, 1, 4, 0))]
DERIVED_CDS = (100, 100)                # the middle third of the 300 nt query


@functools.lru_cache(maxsize=None)
def derived_case():
    """(query, target, jobs): rectangles inside the CDS (k % 3 == 0), outside it (1) and across one of its two boundaries (2),
    near the diagonal of a mutated copy so that the un-annotated paths are made of matches."""
    rng = random.Random(3101)
    q = _rand(rng, 300)
    t = _mutate(rng, q, 0.12) + _rand(rng, 60)
    a, b = DERIVED_CDS[0], DERIVED_CDS[0] + DERIVED_CDS[1]
    jobs = []
    for k in range(300):
        ql, tl = rng.randint(1, 49), rng.randint(2, 49)
        kind = k % 3
        if kind == 0:
            qs = rng.randint(a, b - ql)
        elif kind == 1:
            qs = rng.randint(0, a - ql) if rng.random() < 0.5 else rng.randint(b, len(q) - ql)
        else:
            edge = rng.choice((a, b))
            ql = max(ql, 2)
            qs = rng.randint(edge - ql + 1, edge - 1)                   # qs < edge < qs + ql
        ts = min(max(0, qs + rng.randint(-8, 8)), len(t) - tl)
        jobs.append({"pair": 0, "region": (qs, ts, ql, tl)})
    return q, t, tuple(jobs)


def derived_kind(job):
    """0: inside the CDS, 1: outside (the annotation must change nothing), 2: across a boundary."""
    qs, _, ql, _ = job["region"]
    a, b = DERIVED_CDS[0], DERIVED_CDS[0] + DERIVED_CDS[1]
    if a <= qs and qs + ql <= b:
        return 0
    if qs + ql <= a or qs >= b:
        return 1
    return 2


@functools.lru_cache(maxsize=None)
def derived_oracle(index, annotated):
    """FIND_PATH of every job of derived_case() under DERIVED_MODELS[index] (its score is FIND_SCORE's too)."""
    mt, spec = DERIVED_MODELS[index]
    model = ex.Model.derived(mt, *spec)
    q, t, jobs = derived_case()
    with oracle_annotation(DERIVED_CDS if annotated else None):
        return [oracle_job(model, ex.MODE_FIND_PATH, q, t, j["region"]) for j in jobs]


# ---- long queries: past two strips of query rows (-D 1: checkpoints and continuations) --------------------------------------
# (name, model type, model keyword arguments, query length): the pair shapes of test_seeded_suboptimal_pairs_match_oracle.
# The engine takes a cooperating-wave kernel when a launch has at least three strips of 64 x R rows per job (Engine::run; R = 4:
# 256 rows, so from 512 nt on), and under an annotation only the kernels without the local-scope shortcut remain: affine:local
# has such cooperating-wave kernels (kmw_affine_score, kmw_affine_region, kmw_affine_region_pack), est2genome and ner have none.
# The 520 nt affine:local query is the one that reaches them; the 400 nt ones stay on the one-wave kernels.
LONG_MODELS = [("est2genome", "est2genome", {}, 520), ("affine_local", "affine:local", {}, 400), ("ner", "ner", {}, 400),
               ("affine_local_520", "affine:local", {}, 520)]
# kernels that must be among the launched ones when every variant of that entry runs in one batch at -D 32
LONG_KERNELS = {"affine_local_520": ("kmw_affine_score", "kmw_affine_region_pack")}


def long_cds_variants(qlen):
    """(CDS, may it change the result?): the middle, a range across the first strip boundary's neighbourhood (rows 120-140), one
    across row 256 (the boundary between two strips of four rows per lane), a single position at either end, a negative start
    that still overlaps, a start beyond the query (nothing annotated)."""
    return [((qlen // 3, qlen // 3), True), ((120, 21), True), ((250, 12), True), ((0, 1), True), ((qlen - 1, 1), True),
            ((-10, 30), True), ((qlen + 5, 10), False)]


@functools.lru_cache(maxsize=None)
def long_case(name):
    """(model, query, target) of one LONG_MODELS entry; the target holds the whole query, so both of its ends are aligned."""
    _, mt, kw, qlen = [m for m in LONG_MODELS if m[0] == name][0]
    rng = random.Random(4200 + qlen + len(name))
    q = _rand(rng, qlen)
    if mt == "est2genome":
        c = qlen // 2
        gene = _mutate(rng, q[:c], 0.03) + "GT" + _rand(rng, 400) + "AG" + _mutate(rng, q[c:], 0.03)
        t = _rand(rng, 80) + gene + _rand(rng, 200)             # (that test's second copy of the gene only feeds its later rounds)
    else:
        t = _rand(rng, 30) + _mutate(rng, q, 0.05) + _rand(rng, 90) + _mutate(rng, q, 0.15) + _rand(rng, 20)
    return ex.Model(mt, **kw), q, t


@functools.lru_cache(maxsize=None)
def long_oracle(name, cds, dpmemory):
    model, q, t = long_case(name)
    with oracle_annotation(cds):
        return oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=dpmemory)


# ---- est2genome pairs of about 150 x 600 with a CDS each (run_regions, swap_stage, the shared query buffer) ----------------
def est_pairs(seed, n, qlen=150):
    """[(query, target, cds)]: one intron, flanks, the CDS somewhere inside the query."""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        q = _rand(rng, qlen + 3 * k)
        c = rng.randint(qlen // 3, 2 * qlen // 3)
        t = _rand(rng, 50) + _mutate(rng, q[:c], 0.03) + "GT" + _rand(rng, 250) + "AG" + _mutate(rng, q[c:], 0.03) + _rand(rng, 100)
        start = rng.randint(5, qlen // 2)
        out.append((q, t, (start, rng.randint(20, qlen // 2))))
    return out


def region_cases():
    """[(query, target, cds, region)] for run_regions: each region's query range begins or ends inside the pair's CDS."""
    out = []
    for k, (q, t, cds) in enumerate(est_pairs(5150, 4)):
        mid = cds[0] + cds[1] // 2
        if k % 2 == 0:
            region = (mid, 20, len(q) - mid, len(t) - 30)               # starts inside the CDS
        else:
            region = (0, 0, mid, len(t) - 10 * k)                       # ends inside it
        out.append((q, t, cds, region))
    return out


def oracle_path(model, q, t, cds, dpmemory=32, region=None):
    with oracle_annotation(cds):
        if region is not None:
            return oracle_lib.find_path_region(model.c, model.params, q.encode(), t.encode(), region, dpmemory=dpmemory)
        return oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=dpmemory)
