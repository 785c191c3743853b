"""Generated pairs for coding2coding's SDP (seeded flavour, query advance up to 3), shared by tests/test_sdp_codon_cases.py (what
the bands show, decided on the oracle's alignments), tests/test_sdp_codon_sim.py (the per-lane code driven by CPU loops) and
tests/test_gpu_sdp_codon.py (the kernels): data and plumbing only.

The device passes sweep strips of 64 query rows.  The forward pass's rows are the query positions u, the reverse pass's are
Q - u.  A pair of a band carries ONE handcrafted HSP, so which pass finds which side of the path is known: everything behind
the seed point (the HSP's cobs point) is the forward pass's, everything before it the reverse pass's.  A band b = 64 k,
k = 1 ... 3, holds queries of Q = b - 2 ... b + 3 bases, so that the last strip holds one to six rows, and puts one thing at
the edge of that strip per pair:
  * match: a match (3, 3) that leaves row b - 3, b - 2 or b - 1 (the three frames against the strip), Q = b ... b + 2;
  * q1, q2, qc: a query frameshift of one or two bases, or a codon insert, that leaves a row below b for a row at or above it,
    with one codon behind it (Q = b + 3);
  * t1, t2, tc on row b - 1 or b: a target frameshift / codon delete taken on that row, one codon behind it.  An event on row
    b + 1 needs a codon behind it that ends on row b + 4 > Q, which no query of the band holds: at k >= 2 it is taken at the
    edge before, 64 (k - 1) + 1, by a pair of its own (Q = b - 2 ... b + 3 all the same).
Each of these is built twice: with the HSP in front of it (forward rows) and mirrored, the HSP behind it (reverse rows).  The
events are paid by one W:W codon (11) behind them at the point ALT_FLAGS (every event -9), the default --extensionthreshold.
At dropoff 5 nothing but matches lives: the three frames again, so that along a diagonal only every sixth step of a strip holds
a live cell and, in the frame whose chain sits on rows = b - 3 (mod 3), only the third carried row is live at the edge.
The pairs of k >= 2 are homologous from the query's first codon to its last: the strips in the middle both receive and leave
three carried rows.  A small band holds Q = 3 ... 8 with a one-codon HSP.
"""
import random

import exonerate_amd as ex
import codon_cases as cc
from golden_util import apply_flags

ALT_FLAGS = ["--frameshift", "-9", "--codongapopen", "-9", "--codongapextend", "-2"]
POINTS = {"default": [], "altparams": ALT_FLAGS}
SHAPE = {"match": (3, 3), "q1": (1, 0), "q2": (2, 0), "qc": (3, 0), "t1": (0, 1), "t2": (0, 2), "tc": (0, 3)}
THRESHOLD = 20
BANDS = (1, 2, 3)
_models = {}


def model_at(point):
    if point not in _models:
        _models[point] = ex.Model("coding2coding", params=apply_flags(ex.default_params(), POINTS[point]))
    return _models[point]


def codon_score(params, q, i, t, j):
    return params.protein_submat[cc.codon_code(params, q, i)][cc.codon_code(params, t, j)]


def hsp_of(params, q, t, qs, ts, n):
    """[query_start, target_start, length, score, cobs] of n codons from (qs, ts): the score is the codons' own."""
    return [qs, ts, n, sum(codon_score(params, q, qs + 3 * x, t, ts + 3 * x) for x in range(n)), n // 2]


def _codons(rng, n):
    """n codons of either side for one peptide, synonymous codons drawn apart (only the reading frame they share lines up), no
    W among them (the codon that pays for an event is the only one) and no P (an inserted codon is CCC: beside a P the gap could
    sit on either): [(query codon, target codon)]."""
    return list(zip(*cc._homologous(rng, [rng.choice("ARNDQEGHILKMFSTYV") for _ in range(n)], 0.0))) if n else []


def edge_pair(rng, kind, row, qlen, mirrored):
    """One pair of a band: blocks [flank][homologous codons, the HSP its first][event][TGG, the codon that pays, and as many
    homologous codons as the query still holds][0-2 bases] (a plain match chain: no event, no W), read as they stand or,
    mirrored, last block first with each block's codons last first.  `row`: the row the event's transition leaves -- for "match"
    the row the chain's last match leaves -- in the rows of the pass that finds it."""
    aq, at = SHAPE[kind]
    flank = row % 3
    if kind == "match":
        assert qlen == row + 3
        hom, tail, ev_q, ev_t, fill = _codons(rng, row // 3 + 1), [], "", "", ""
    else:
        more = qlen - (row + aq + 3)
        assert more >= 0, (kind, row, qlen)
        hom, tail, fill = _codons(rng, row // 3), [("TGG", "TGG")] + _codons(rng, more // 3), cc._dna(rng, more % 3)
        ev_q, ev_t = "C" * aq, "C" * at                         # (C, CC, CCC: no codon they start scores above 0 against W)
        # the codon in front of the event is TGT (C, 9 against itself): moved across it the event would pair it with GTC, TCC, CCC,
        # CTG or CCT (V, S, P, L, P: -1 at best), so the event has one place
        hom[-1] = ("TGT", "TGT")
    n_hsp = min(6, len(hom))
    qb = [cc._dna(rng, flank), hom, ev_q, tail, fill]
    tb = [cc._dna(rng, rng.randint(3, 12)), hom, ev_t, tail, cc._dna(rng, rng.randint(3, 12))]
    hsp_at = 0
    if mirrored:
        qb = [qb[4], qb[3][::-1], qb[2], qb[1][::-1], qb[0]]
        tb = [tb[4], tb[3][::-1], tb[2], tb[1][::-1], tb[0]]
        hsp_at = len(hom) - n_hsp
    text = lambda blocks, side: "".join(x if isinstance(x, str) else "".join(c[side] for c in x) for x in blocks)
    at_hom = 3 if mirrored else 1                               # where the homologous block now stands
    q, t = text(qb, 0), text(tb, 1)
    assert len(q) == qlen, (len(q), qlen)
    return dict(q=q, t=t, kind=kind, row=row, mirrored=mirrored,
                hsp_blocks=(len(text(qb[:at_hom], 0)) + 3 * hsp_at, len(text(tb[:at_hom], 1)) + 3 * hsp_at, n_hsp))


def band_pairs(k):
    """The pairs of band k (1 ... 3), a fixed seed: (pairs at the default dropoff, pairs at dropoff 5)."""
    rng = random.Random("codon sdp band %d" % k)
    b = 64 * k
    wide, drop = [], []
    for mirrored in (False, True):
        for row in (b - 5, b - 4, b - 3, b - 2, b - 1):        # Q = b - 2, b - 1: the strip before is (all but) full, no row behind it
            wide.append(edge_pair(rng, "match", row, row + 3, mirrored))
            if row >= b - 3:
                drop.append(edge_pair(rng, "match", row, row + 3, mirrored))
        for kind in ("q1", "q2", "qc"):
            wide.append(edge_pair(rng, kind, b - SHAPE[kind][0], b + 3, mirrored))
        for n, kind in enumerate(("t1", "t2", "tc")):
            for row in (b - 1, b):
                wide.append(edge_pair(rng, kind, row, row + 3, mirrored))
            if k >= 2:                                          # row 64 (k - 1) + 1: see the head of this file
                wide.append(edge_pair(rng, kind, b - 63, b - 2 + (2 * n + k + mirrored) % 6, mirrored))
    return wide, drop


def small_pairs():
    """Q = 3 ... 8 with a one-codon HSP (forward and mirrored): fewer rows than two advances."""
    rng = random.Random("codon sdp small")
    out = []
    for qlen in range(3, 9):
        for mirrored in (False, True):
            n = qlen // 3
            hom = ["TGG"] * n
            flank = cc._dna(rng, qlen - 3 * n)
            tfl = cc._dna(rng, rng.randint(0, 4))
            q = "".join(hom) + flank if mirrored else flank + "".join(hom)
            t = tfl + "".join(hom) + cc._dna(rng, rng.randint(0, 4))
            at = (n - 1) if mirrored else 0
            out.append(dict(q=q, t=t, kind="match", row=None, mirrored=mirrored,
                            hsp_blocks=((0 if mirrored else len(flank)) + 3 * at, len(tfl) + 3 * at, 1)))
    return out


def hsps_of(params, pair):
    qs, ts, n = pair["hsp_blocks"]
    return [hsp_of(params, pair["q"], pair["t"], qs, ts, n)]


def walk(model, aln):
    """(query position, target position, query advance, target advance) of every transition of alignment dict `aln`."""
    i, j = aln["region"][0], aln["region"][1]
    for tr, length in aln["ops"]:
        t = model.c.transitions[tr]
        for _ in range(length):
            yield i, j, t.advance_query, t.advance_target
            i += t.advance_query
            j += t.advance_target


def shows(model, pair, hsp, alns):
    """None when the oracle's alignments of `pair` take the pair's event on its row in the rows of the pass that must find it
    (behind the seed point: forward rows u; before it: reverse rows Q - u), else a line that says what was seen."""
    if pair["row"] is None:
        return None if alns else "no alignment"
    Q = len(pair["q"])
    seed_q = hsp[0] + 3 * hsp[4]
    want = SHAPE[pair["kind"]]
    seen = []
    for a in alns:
        for i, j, aq, at in walk(model, a):
            if (aq, at) != want:
                continue
            if not pair["mirrored"] and i >= seed_q:
                seen.append(i)
            if pair["mirrored"] and i + aq <= seed_q:
                seen.append(Q - (i + aq))
    if pair["kind"] == "match":
        ok = pair["row"] in seen and max(seen) == pair["row"]       # ... and it is the chain's last
    else:
        ok = seen == [pair["row"]]
    return None if ok else "%s %s row %d (Q = %d): taken on rows %r" % (
        pair["kind"], "reverse" if pair["mirrored"] else "forward", pair["row"], Q, seen)


def band_runs(k):
    """What band k (1 ... 3, or "small") is run as: [(parameter point, dropoff, pair)].  The events at the point ALT_FLAGS, the
    match chains at both points, all at the default dropoff; the three frames again at dropoff 5."""
    if k == "small":
        return [(point, 50, p) for point in POINTS for p in small_pairs()]
    wide, drop = band_pairs(k)
    return [("altparams", 50, p) for p in wide] + [("default", 50, p) for p in wide if p["kind"] == "match"] + \
           [("default", 5, p) for p in drop]


_oracle = {}


def oracle_sdp(model, q, t, hsps, adv, dropoff, threshold, n=4):
    """The oracle's alignments of one pair, computed once per test session and left alone."""
    import oracle_lib
    key = (id(model), q, t, repr(hsps), adv, dropoff, threshold, n)
    if key not in _oracle:
        ub, alns = oracle_lib.sdp(model.c, model.params, q.encode(), t.encode(), hsps, adv[0], adv[1], dropoff, True, threshold, n)
        assert ub == 0
        _oracle[key] = alns
    return _oracle[key]


# ---- seeded fuzz ----------------------------------------------------------------------------------------------------------
def _codon_hsps(params, q, t, w=4, dropoff=12, threshold=25):
    """HSPs with advances 3/3 (the comparison's codon set): every shared word of w residues, any frames, grown without gaps
    until the score falls `dropoff` below its maximum; one HSP per stretch of a diagonal.  SDP takes them as seed points."""
    code_q = [cc.codon_code(params, q, i) if i + 3 <= len(q) else -1 for i in range(len(q))]
    code_t = [cc.codon_code(params, t, j) if j + 3 <= len(t) else -1 for j in range(len(t))]
    sm = params.protein_submat
    words = {}
    for i in range(len(q) - 3 * w + 1):
        words.setdefault(tuple(code_q[i + 3 * x] for x in range(w)), []).append(i)
    covered, out = {}, []
    for j in range(len(t) - 3 * w + 1):
        for i in words.get(tuple(code_t[j + 3 * x] for x in range(w)), ()):
            d = (j - i, i % 3)
            if covered.get(d, -1) >= i:
                continue
            lo, best, run = 0, 0, 0
            x = 1
            while i - 3 * x >= 0 and j - 3 * x >= 0 and run - best > -dropoff:
                run += sm[code_q[i - 3 * x]][code_t[j - 3 * x]]
                if run > best:
                    best, lo = run, x
                x += 1
            hi, best, run = 0, 0, 0
            x = 0
            while i + 3 * x + 3 <= len(q) and j + 3 * x + 3 <= len(t) and run - best > -dropoff:
                run += sm[code_q[i + 3 * x]][code_t[j + 3 * x]]
                if run > best:
                    best, hi = run, x + 1
                x += 1
            qs, ts, n = i - 3 * lo, j - 3 * lo, lo + hi
            covered[d] = qs + 3 * n
            score = sum(sm[code_q[qs + 3 * y]][code_t[ts + 3 * y]] for y in range(n))
            if n and score >= threshold:
                out.append([qs, ts, n, score, n // 2])
    return out


def _dna_hsps(params, q, t, w=10):
    import oracle_lib
    words = {}
    for i in range(len(q) - w + 1):
        words.setdefault(q[i:i + w], []).append(i)
    seeds = [(i, j) for j in range(len(t) - w + 1) for i in words.get(t[j:j + w], ())]
    return oracle_lib.hsp_set(params, "dna2dna", q.encode(), t.encode(), w, 30, 30, seeds) if seeds else []


def fuzz_pair(rng, qmax):
    """A homologous coding pair: nine codons in ten kept, up to three events (frameshifts of one, two, four or five bases, gaps of
    one to three codons) on either axis, flanks; now and then a second copy of the body in the target."""
    top = max(1, qmax // 3)
    ncod = rng.choice((rng.randint(1, min(6, top)), rng.randint(min(8, top), min(40, top)), rng.randint(min(40, top), top)))
    qc = [rng.choice(cc.CODONS[rng.choice(cc.AA)]) for _ in range(ncod)]
    tc = [c if rng.random() < 0.9 else rng.choice(cc.CODONS[rng.choice(cc.AA)]) for c in qc]
    for _ in range(rng.choice((0, 1, 1, 2, 3))):
        side = qc if rng.random() < 0.5 else tc
        side.insert(rng.randrange(len(side) + 1), cc._dna(rng, rng.choice((1, 2, 3, 4, 5, 6, 9))))
    q = (cc._dna(rng, rng.randint(0, 8)) + "".join(qc) + cc._dna(rng, rng.randint(0, 8)))[:qmax]
    body = "".join(tc)
    t = cc._dna(rng, rng.randint(0, 40)) + body + cc._dna(rng, rng.randint(0, 40))
    if rng.random() < 0.3:
        t += body[len(body) // 3:] + cc._dna(rng, 9)
    return q, t


def fuzz_cases(seed, rounds=4, pairs_per_round=6, qmax=330):
    """Seeded random batches: advances 1/1 with DNA-style seed points and 3/3 with codon HSPs, several seeds per pair, dropoff 5
    and 50, both parameter points, queries of 3 to qmax bases."""
    rng = random.Random(7100 + seed)
    out = []
    for r in range(rounds):
        point = ("default", "altparams")[(seed + r) % 2]
        model = model_at(point)
        adv = ((1, 1), (3, 3))[(seed + r // 2) % 2]
        dropoff = (5, 50)[r % 2]
        pairs, hsps = [], []
        for k in range(pairs_per_round):
            q, t = fuzz_pair(rng, qmax if k else 3 + 3 * r)
            q = q if len(q) >= 3 else "TGG"
            h = _dna_hsps(model.params, q, t) if adv == (1, 1) else _codon_hsps(model.params, q, t)
            if not h and len(q) < 12:                          # too short for a word: a seed point all the same
                h = [hsp_of(model.params, q, q + t, 0, 0, 1)]
                t = q + t
            if h:
                pairs.append((q, t)); hsps.append(h)
        if pairs:
            out.append(dict(model=model, point=point, pairs=pairs, hsps=hsps, adv=adv, dropoff=dropoff, threshold=rng.choice((30, 60))))
    return out
