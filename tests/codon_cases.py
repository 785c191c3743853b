"""The vector sets of the translated models -- ungapped:trans (src/model/ungapped.c:106-166 with Match_Type_CODON2CODON) and
coding2coding (src/model/coding2coding.c:50-66) -- and their loaders, shared by the codon tests (data and plumbing only; no
reference code).  Both kinds are made by tools/make_golden.py:
  * refdump-made (tests/golden/coding2coding*.jsonl, ungapped_trans*.jsonl): records of the reference's Optimal_find_score /
    Optimal_find_path, default parameters and the point CODONALT_FLAGS, -D 32 and -D 0, with the sub-optimal loop.
  * reference-binary-made (tests/golden/codon_cli_*.json): inputs and stdout of `exonerate --model <m> --exhaustive yes --subopt no
    -n 1` with every report switched on, one run per pair, two of them with their best alignment on a minus strand; beside each,
    the same alignment as transition ids (refdump on the strands the binary chose).
The CPU oracle restates the 3:3 match (oracle/c4_oracle.c, C4GPU_CALC_MATCH_CODON) and is pinned on all of these records and, at
sizes they do not reach, on refdump run on the spot (tests/test_oracle_codon.py); the generators at the end of this file make the
pairs of that live check and of the device tests that are held to the oracle (tests/test_gpu_codon_oracle.py).
"""
import json, os, random

import exonerate_amd as ex
from exonerate_amd import _abi
from golden_util import GOLDEN_DIR, apply_flags, load_set

CODONALT_FLAGS = ["--codongapopen", "-11", "--codongapextend", "-3", "--frameshift", "-13", "--proteinsubmat", "pam250"]
# set -> model type
REFDUMP_SETS = {"coding2coding": "coding2coding", "coding2coding_D0": "coding2coding",
                "coding2coding_codonalt": "coding2coding", "coding2coding_codonalt_D0": "coding2coding",
                "ungapped_trans": "ungapped:trans", "ungapped_trans_D0": "ungapped:trans", "ungapped_trans_codonalt": "ungapped:trans"}
# ... with the GAM sub-optimal loop (rec["subopt"], rec["threshold"]; --suboptmax 4)
SUBOPT_SETS = {"coding2coding_subopt": "coding2coding", "coding2coding_subopt_D0": "coding2coding",
               "ungapped_trans_subopt": "ungapped:trans"}
CLI_SETS = ["codon_cli_coding2coding", "codon_cli_coding2coding_alt", "codon_cli_ungapped_trans"]
SUBOPT_MAX = 4
MODEL_NAME = {"coding2coding": "coding2coding", "ungapped:trans": "ungapped:codon"}


def set_model(name):
    mt = REFDUMP_SETS[name] if name in REFDUMP_SETS else SUBOPT_SETS[name]
    params = ex.default_params()
    if "_codonalt" in name:
        apply_flags(params, CODONALT_FLAGS)
    return ex.Model(mt, params=params)


def load_cli(name):
    """(set, model): the recorded runs of one parameter point and the model at that point."""
    with open(os.path.join(GOLDEN_DIR, name + ".json")) as f:
        data = json.load(f)
    return data, ex.Model(data["model"], params=apply_flags(ex.default_params(), data["flags"]))


_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def strand_seqs(pair):
    """The two sequences as the recorded alignment reads them (a minus strand: reverse-complemented)."""
    q = revcomp(pair["query"]) if pair["qstrand"] == "-" else pair["query"]
    t = revcomp(pair["target"]) if pair["tstrand"] == "-" else pair["target"]
    return q, t


def cli_lines(data, pair, aln):
    """The stdout lines of the recorded run of `pair`, printed by the library's printers for alignment `aln` (an
    exonerate_amd.Alignment, whoever computed it), without the ##date line the recording dropped."""
    q, t = strand_seqs(pair)
    qid, tid, qs, ts = pair["id"], pair["tid"], pair["qstrand"], pair["tstrand"]
    qdef = pair["qdef"] + (":[revcomp]" if qs == "-" else "")
    tdef = "[revcomp]" if ts == "-" else None
    text = aln.display(q, t, qid, tid, qs, ts, qdef=qdef, tdef=tdef)
    text += aln.sugar(qid, tid, qs, ts) + "\n" + aln.cigar(qid, tid, qs, ts) + "\n"
    text += aln.vulgar(qid, tid, qs, ts) + "\n"
    text += aln.gff(q, t, qid, tid, qs, ts, on_query=True, result_id=0)
    text += aln.gff(q, t, qid, tid, qs, ts, on_query=False, result_id=0)
    text += aln.ryo(data["ryo"], q, t, qid, tid, qs, ts, qdef=qdef, tdef=tdef)
    text += "-- completed exonerate analysis\n"
    return [l for l in text.split("\n") if not l.startswith("##date ")]


def recorded_alignment(model, pair):
    """The recorded alignment of a reference-binary-made pair as an exonerate_amd.Alignment (the printers need no device)."""
    return ex.Alignment.from_parts(model, pair["score"], pair["region"], pair["ops"], len(pair["query"]), len(pair["target"]))


def codon_code(params, seq, pos):
    """Substitution-matrix row of the residue that seq[pos:pos + 3] encodes (Translate_base, translate.h:73-76, then Submat's
    index), from the tables the parameter block carries."""
    a, b, c = (params.nt2d[ord(x)] for x in seq[pos:pos + 3])
    return params.submat_index[params.aa[params.trans[a | (b << 4) | (c << 8)]]]


def replay(model, rec):
    """Walks rec["ops"] through the model's transition table: (score, query advance, target advance, labels seen), asserting
    that the ids chain from START to END.  The match calc is protein_submat[aa(q[i..i+2])][aa(t[j..j+2])] (match.c:508-530)."""
    m, p = model.c, model.params
    qs, ts = rec["region"][0], rec["region"][1]
    i, j, score, state, labels = qs, ts, 0, m.start_state, set()
    for tr, length in rec["ops"]:
        t = m.transitions[tr]
        for _ in range(length):
            assert t.input == state, (rec["id"], tr, state)
            if t.calc >= 0:
                c = m.calcs[t.calc]
                if c.kind == _abi.CALC_MATCH_CODON:
                    score += p.protein_submat[codon_code(p, rec["query"], i)][codon_code(p, rec["target"], j)]
                else:
                    assert c.kind == _abi.CALC_CONST
                    score += c.value
            i += t.advance_query
            j += t.advance_target
            state = t.output
            labels.add(t.label)
    assert state == m.end_state, rec["id"]
    return score, i - qs, j - ts, labels


# ---- generated pairs: strip and lane edges, fuzz ---------------------------------------------------------------------
# every event (frameshift, codon gap) costs less than one W:W codon, 11, scores: the path takes it with one codon left
CHEAP_FLAGS = ["--frameshift", "-9", "--codongapopen", "-9", "--codongapextend", "-2"]
POINTS = {"default": [], "cheap": CHEAP_FLAGS, "codonalt": CODONALT_FLAGS}
HUGE_FLAGS = ["--frameshift", "-350000000"]      # (3.5e8 + 11) x (7 states + 4) > 4e8: Engine::local_exact goes off by itself
ALL_POINTS = dict(POINTS, huge=HUGE_FLAGS)
EDGE_POINTS = {"coding2coding": ("cheap", "default"), "ungapped:trans": ("default", "codonalt")}
STRIP = 256                     # query rows of one strip (64 lanes x R = 4 rows, c4_viterbi_kernel.h)
BANDS = ("small", 1, 2, 3, 4)
AA = "ARNDCQEGHILKMFPSTWYV"
_NCBI = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODONS = {}
for _i, _a in enumerate("TCAG"):
    for _j, _b in enumerate("TCAG"):
        for _k, _c in enumerate("TCAG"):
            CODONS.setdefault(_NCBI[_i * 16 + _j * 4 + _k], []).append(_a + _b + _c)


def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _homologous(rng, pep, rate=0.1):
    """Two codon lists for one peptide: synonymous codons drawn apart, `rate` of the target's residues replaced."""
    return ([rng.choice(CODONS[a]) for a in pep],
            [rng.choice(CODONS[rng.choice(AA) if rng.random() < rate else a]) for a in pep])


def _edge_pair(rng, qlen, flank, near, far=None, tail_w=False):
    """A query of exactly qlen bases: `flank` random bases, then codons to its end (the last 0-2 bases random), against a
    target that encodes nearly the same peptide between 20-75 random bases on either side.  `near` and `far` are events
    (kind, query offset): kind q1 / q2 / qc puts one base, two bases or one codon into the query so that they begin at the first
    codon boundary at or after the offset; t1 / t2 / tc puts them into the target across from that boundary.  tail_w: the pair
    begins with one codon that is the same on both sides (the alignment starts at the query's first codon) and the query ends in
    TGG on both sides right in front of and right behind the last event (a W:W match, 11, pays for one event of the cheap point
    and for nothing dearer, and no other place for the event scores as much)."""
    events = sorted([e for e in (near, far) if e is not None], key=lambda e: e[1])
    q, t = [_dna(rng, flank)], [_dna(rng, rng.randint(20, 75))]
    have = flank

    def codons(n):
        qc, tc = _homologous(rng, [rng.choice(AA) for _ in range(n)])
        q.extend(qc)
        t.extend(tc)

    if tail_w:
        q.append("TGG")
        t.append("TGG")
        have += 3
    for kind, at in events:
        n = max(0, -(-(at - have) // 3))                  # codons up to the first boundary at or after `at`
        n = min(n, (qlen - have) // 3)
        if tail_w and (kind, at) == events[-1] and n:     # W:W in front of the last event as well: no other place for it scores as much
            codons(n - 1)
            q.append("TGG")
            t.append("TGG")
        else:
            codons(n)
        have += 3 * n
        extra = {"1": 1, "2": 2, "c": 3}[kind[1]]
        if kind[0] == "q":
            if have + extra > qlen:
                continue
            q.append("C" * extra if tail_w else _dna(rng, extra))       # (C, CC, CCC: no codon they start scores above 0 against W)
            have += extra
        else:
            t.append("C" * extra if tail_w else _dna(rng, extra))
    if tail_w:
        assert have + 3 == qlen, (have, qlen)
        q.append("TGG")
        t.append("TGG")
        have += 3
    else:
        n = (qlen - have) // 3
        keep = min(n, 3)
        codons(n - keep)
        same = [rng.choice(CODONS[rng.choice(AA)]) for _ in range(keep)]          # the alignment runs to the query's last codon
        q.extend(same)
        t.extend(same)
        have += 3 * n
        q.append(_dna(rng, qlen - have))
    t.append(_dna(rng, rng.randint(20, 75)))
    q, t = "".join(q), "".join(t)
    assert len(q) == qlen
    return q, t


def _small_pairs(model_type, rng):
    """Query lengths 1 ... 13 against targets of 1 ... 20: fewer rows than an advance, and the lane edges at multiples of 4."""
    out = []
    for qlen in range(1, 14):
        flank = qlen % 3 if qlen >= 6 else 0
        n = (qlen - flank) // 3
        qc, tc = _homologous(rng, [rng.choice("WCFYHM") for _ in range(n)], 0.0)
        q = _dna(rng, flank) + "".join(qc)
        q += _dna(rng, qlen - len(q))
        t = _dna(rng, rng.randint(0, 2)) + "".join(tc)
        if model_type == "coding2coding" and n >= 3 and qlen % 2:
            t = t[:len(t) - 3] + rng.choice("ACGT") + t[len(t) - 3:]               # a target frameshift in front of the last codon
        tlen = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 19, 20)[qlen - 1]
        t = (t + _dna(rng, 20))[:tlen] if qlen < 4 or tlen < len(t) else t + _dna(rng, max(0, tlen - len(t)))
        out.append((q, t[:20]))
    return out


# kind -> (query advance, target advance) of the transition that takes the event
EVENT_SHAPE = {"q1": (1, 0), "q2": (2, 0), "qc": (3, 0), "t1": (0, 1), "t2": (0, 2), "tc": (0, 3)}
# kind -> (query row at which the event's transition starts, less 256 k; query length, less 256 k): behind the event the query
# holds one more codon, so the target-side events decide the length
_AT_EDGE = {"t1": (-3, 0), "tc": (-2, 1), "t2": (-1, 2), "q1": (-1, 3), "q2": (-2, 3), "qc": (-3, 3)}


def edge_pairs(model_type, k, rng):
    """The band of strip boundary 256 k: homologous coding pairs whose queries are 256 k - 2 ... 256 k + 3 bases long, so that the
    last strip holds one to four rows (row 0 is the empty prefix), with flanks of 0-2 bases, so that the frame takes all three
    values.  coding2coding: three plain pairs (256 k - 2, 256 k - 1 and 256 k + 3 bases) with one event on either axis at an
    earlier boundary 256 j or mid-query, and one pair for each of the six events -- a one-base, a two-base and a codon insertion
    in the query (q1, q2, qc) and in the target (t1, t2, tc) -- whose transition starts at query row 256 k - 3 ... 256 k - 1 and,
    on the query side, ends on row 256 k.  So short a query holds one codon behind such an event, so the path takes it only where
    it costs less than that codon can score: the pair ends in W:W (11) and the point is CHEAP_FLAGS (every event -9).  The
    query-side pairs have no flank and an earlier query insertion that sets their frame, so their alignments start at row 0 and the
    boundary is the same counted from the query's start (the score and region passes) and from the region's (the path passes).
    k = "small": see _small_pairs."""
    if k == "small":
        return _small_pairs(model_type, rng)
    b = STRIP * k
    out = []
    if model_type == "ungapped:trans":
        for qlen in range(b - 2, b + 4):
            out.append(_edge_pair(rng, qlen, qlen % 3 if qlen != b + 3 else rng.randint(0, 2), None))
        return out
    for n, qlen in enumerate((b - 2, b - 1, b + 3)):
        inner = STRIP * rng.randint(1, k - 1) if k > 1 else 120
        kind = ("q1", "t2", "qc", "t1", "q2", "tc")[(n + 3 * k) % 6]
        other = {"q": "t", "t": "q"}[kind[0]] + rng.choice("12c")
        out.append(_edge_pair(rng, qlen, rng.randint(0, 2), (kind, inner - 3 + rng.randint(0, 6)),
                              (other, inner - 45 + rng.randint(0, 6))))
    for kind, (at, qlen) in _AT_EDGE.items():
        at, qlen = b + at, b + qlen
        if kind[0] == "t":
            n = rng.randint(1, 3)                                                  # an earlier query insertion, and the flank that fits it
            out.append(_edge_pair(rng, qlen, (at - n) % 3, (kind, at), ("q" + "12c"[n - 1], b - 90), tail_w=True))
        else:
            fix = ("q%d" % (at % 3), b - 90) if at % 3 else ("t" + rng.choice("12c"), b - 90)
            out.append(_edge_pair(rng, qlen, 0, (kind, at), fix, tail_w=True))
    return out


def _walk(model, aln):
    """(query row, query advance, target advance) of every transition of alignment dict `aln`."""
    if aln is None:
        return
    i = aln["region"][0]
    for tr, length in aln["ops"]:
        t = model.c.transitions[tr]
        for _ in range(length):
            yield i, t.advance_query, t.advance_target
            i += t.advance_query


def crossings(model, aln, boundary, from_region_start=False):
    """{(query advance, rows past the boundary)} of the transitions of alignment dict `aln` that go from a query row below
    `boundary` to one at or above it; from_region_start: rows counted from the alignment's first row, as the path passes do."""
    if aln is not None and from_region_start:
        boundary += aln["region"][0]
    return {(a, i + a - boundary) for i, a, _ in _walk(model, aln) if a and i < boundary <= i + a}


def events_at(model, aln, boundary):
    """The kinds of EVENT_SHAPE whose transition starts at a query row boundary - 3 ... boundary + 3 in alignment dict `aln`."""
    kinds = {shape: kind for kind, shape in EVENT_SHAPE.items()}
    return {kinds[(a, d)] for i, a, d in _walk(model, aln) if (a, d) in kinds and boundary - 3 <= i <= boundary + 3}


def required_crossings(model_type):
    """What a band k = 1 ... 4 must show at its boundary 256 k, in the oracle's alignments, over its parameter points."""
    if model_type == "ungapped:trans":
        return {(3, 0), (3, 1), (3, 2)}
    return {(1, 0), (2, 0), (3, None)}


def crossings_hold(model_type, seen_by_point):
    """seen_by_point: parameter point -> crossings() of the band's alignments at that point.  Every point must show an advance
    of 3 across the boundary; the rest of required_crossings may come from any point."""
    seen = set().union(*seen_by_point.values())
    need = required_crossings(model_type)
    return all(any(x[0] == 3 for x in s) for s in seen_by_point.values()) and \
        all(((a, o) in seen) if o is not None else any(x[0] == a for x in seen) for a, o in need)


def band_shows(model_type, k, alns_by_point):
    """Everything a band k = 1 ... 4 must show, decided on alignment dicts {parameter point: [alignment of each pair]} (the
    oracle's): None, or a line that says what is missing.
      * crossings_hold at 256 k in the query's own rows (the strips of the score and region passes);
      * the same counted from each alignment's first row (the strips of the path, checkpoint and continuation passes), at
        256 k for coding2coding -- an advance of 1, of 2 and of 3 -- and at every 256 j, j <= k, for ungapped:trans, where an
        advance of 3 lands (-j) mod 3 rows past it whatever the pair: k = 4 shows all of {0, 1, 2};
      * coding2coding, at the point "cheap": every event of EVENT_SHAPE is taken at a row 256 k - 3 ... 256 k + 3."""
    b = STRIP * k
    models = {p: point_model(model_type, p) for p in alns_by_point}
    seen = {p: set().union(*[crossings(models[p], a, b) for a in alns]) for p, alns in alns_by_point.items()}
    if not crossings_hold(model_type, seen):
        return "rows of the query, 256 x %s: %r" % (k, seen)
    if model_type == "ungapped:trans":
        rel = {j: set().union(*[crossings(models[p], a, STRIP * j, True) for p, alns in alns_by_point.items() for a in alns])
               for j in range(1, k + 1)}
        if any(rel[j] != {(3, -j % 3)} for j in range(1, k)) or not rel[k] <= {(3, -k % 3)}:
            return "rows of the region, ungapped:trans: %r" % (rel,)
        return None
    rel = set().union(*[crossings(models[p], a, b, True) for p, alns in alns_by_point.items() for a in alns])
    if not {1, 2, 3} <= {a for a, _ in rel}:
        return "rows of the region, 256 x %s: %r" % (k, rel)
    events = set().union(*[events_at(models["cheap"], a, b) for a in alns_by_point["cheap"]])
    if events != set(EVENT_SHAPE):
        return "events at 256 x %s - 3 ... + 3: only %r" % (k, sorted(events))
    return None


def fuzz_pair(rng):
    """Homologous coding sequences of one, two, three and five strips (up to about 1 400 bases): substitutions, codon indels, one-
    and two-base frameshifts on either axis, flanks of 0 to 5 bases, now and then an N, an ambiguity code, a stop codon or lower
    case; some targets carry a second, mutated copy of the body, so that sub-optimal rounds find something."""
    n = rng.choice([rng.randint(1, 12), rng.randint(20, 80), rng.randint(90, 160), rng.randint(180, 250), rng.randint(350, 460)])
    pep = [rng.choice(AA) for _ in range(n)]
    qc = [rng.choice(CODONS[a]) for a in pep]
    tc = [rng.choice(CODONS[rng.choice(AA + "*") if rng.random() < 0.1 else a]) for a in pep]
    for side in (qc, tc):
        for _ in range(rng.choice([0, 1, 2, 3])):
            at = rng.randrange(len(side))
            kind = rng.randrange(4)
            if kind == 0:
                side[at:at] = [rng.choice(CODONS[rng.choice(AA)]) for _ in range(rng.randint(1, 3))]
            elif kind == 1 and len(side) > 1:
                del side[at]
            elif kind == 2:
                side[at] += _dna(rng, rng.randint(1, 2))
            elif len(side[at]) == 3:
                side[at] = side[at][:rng.randint(1, 2)]
    q, body = "".join(qc), "".join(tc)
    t = body
    if rng.random() < 0.3:
        copy = "".join(rng.choice("ACGT") if rng.random() < 0.06 else c for c in body)
        t = body + _dna(rng, rng.randint(7, 50)) + copy[rng.randint(0, 2):]
    out = []
    for s in (q, t):
        s = _dna(rng, rng.randint(0, 5)) + s + _dna(rng, rng.randint(0, 5))
        if rng.random() < 0.25:
            s = "".join(rng.choice("NRYKMSW") if rng.random() < 0.03 else c for c in s)
        if rng.random() < 0.2:
            s = s.lower() if rng.random() < 0.5 else s[:len(s) // 2] + s[len(s) // 2:].lower()
        out.append(s or "A")
    return tuple(out)


def band_rng(model_type, k):
    """The fixed seed of a band: the live check against the reference and the device tests draw the same pairs."""
    return random.Random("%s/%s" % (model_type, k))


def point_model(model_type, point):
    return ex.Model(model_type, params=apply_flags(ex.default_params(), ALL_POINTS[point]))


__all__ = ["REFDUMP_SETS", "SUBOPT_SETS", "CLI_SETS", "SUBOPT_MAX", "CODONALT_FLAGS", "MODEL_NAME", "set_model", "load_cli",
           "cli_lines", "recorded_alignment", "strand_seqs", "revcomp", "replay", "codon_code", "load_set", "_abi", "CHEAP_FLAGS",
           "POINTS", "ALL_POINTS", "HUGE_FLAGS", "EDGE_POINTS", "BANDS", "STRIP", "edge_pairs", "fuzz_pair", "crossings", "crossings_hold", "events_at", "band_shows",
           "EVENT_SHAPE", "band_rng",
           "point_model"]
