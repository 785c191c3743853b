"""Pairs that put something on a strip, workgroup, chunk or dump boundary of the kernels of the one-row-advance families --
affine (four scopes, DNA and protein), ner, est2genome, protein2dna, protein2genome -- and the claims each pair makes about the
oracle's alignment of it (data and plumbing only; no reference code).  The sibling of codon_cases.edge_pairs for the families
whose transitions advance the query by one row.

Geometry.  Nothing here knows a strip height: a FORM is a set of C4GPU_* switches and the launches they lead to, and
form_boundaries() asks the kernel table (tests/kernel_choice_sim_lib.geometry: KernelInfo::R, waves, hbm_carry,
pk16_staged_rows / _rows6) for the rows per lane and waves per job of the kernel that serves each launch; a form's row boundaries
are its strip height 64 R and its workgroup height waves x 64 R (the staged packed forms: the staged rows; PK16_STAGED_LONG: its
super-strip), and its BANDS are those of ROW_BANDS that fall on one of them.

Row origins.  The score and region passes, the region windows (c4_win16_kernel.h: "window rows are lattice rows: a window starts
in row 0") and the dumping score pass count rows from the query's first row; the path, checkpoint and continuation passes (and the
packed checkpoint pass, c4_ckpt16_kernel.h: it "runs from the region's start to its end cell") from the region's first row.  Every
event pair has no query flank and begins with identical residues on both sides, so its alignment starts at query row 0 and one
boundary serves both origins; the pairs whose region starts on the edge (start_pairs) and the ties are claims about the query's
own rows alone.

A pair is a dict {"q", "t", "claims"}; a claim is a tuple that pair_shows() decides on the oracle's alignment:
  ("event", kind, row)     an event of EVENT_KINDS whose first transition starts at query row `row`
  ("start", row)           the alignment begins at query row `row`
  ("end_col", col)         ... and ends at target column `col`
  ("intron_from", col) / ("intron_to", col) / ("intron_over", col)    an intron begins at / ends at / covers target column `col`
  ("tie_rows", a, b) / ("tie_cols", a, b)   the whole pair scores what the query (target) cut behind a and cut in front of b scores
"""
import random

import exonerate_amd as ex
from exonerate_amd import _abi
from golden_util import apply_flags
from codon_cases import crossings, revcomp, CODONS
import oracle_lib

# every row boundary a form of the table has today falls on one of these: 768 = lcm(128, 192, 256, 384); 1 024 and 1 536 are the
# workgroup heights of the 4 x 256 / 8 x 128 forms and of the six-row forms (staged rows, super-strip)
ROW_BANDS = (64, 128, 192, 256, 384, 512, 768, 1024, 1536)
# chunk edges of the cooperating waves (64 columns), the wrap of their 256-column ring, and -- at C4GPU_SEED_KSHIFT 5 / 6 -- dump
# columns of the two-pass region search
COL_BANDS = (64, 128, 192, 256, 320)

# ---- families ---------------------------------------------------------------------------------------------------------------
# key -> (model type, query alphabet, target alphabet); the parameter point "cheap": a gap of three costs less than one mismatch each
CHEAP_GAPS = ["--gapopen", "-2", "--gapextend", "-1"]
FAMILIES = {
    "affine:local/dna": ("affine:local", 0, 0), "affine:global/dna": ("affine:global", 0, 0),
    "affine:bestfit/dna": ("affine:bestfit", 0, 0), "affine:overlap/dna": ("affine:overlap", 0, 0),
    "affine:local/protein": ("affine:local", 1, 1), "affine:global/protein": ("affine:global", 1, 1),
    "ner/dna": ("ner", 0, 0), "est2genome": ("est2genome", 0, 0), "protein2dna": ("protein2dna", 1, 0),
    "protein2genome": ("protein2genome", 1, 0),
}
_MODELS = {}


def family_model(family, point="default"):
    """The model of a family at a parameter point: "default", or "cheap" (CHEAP_GAPS: the pair of the gap taken on either axis)."""
    key = (family, point)
    if key not in _MODELS:
        mt, qa, ta = FAMILIES[family]
        params = apply_flags(ex.default_params(), CHEAP_GAPS if point == "cheap" else [])
        _MODELS[key] = ex.Model(mt, qa, ta, params=params)
    return _MODELS[key]


def kernel_family(family):
    """The kernel family (kernel_choice_sim_lib.FAMILY) of a key of FAMILIES."""
    return family.split(":")[0].split("/")[0]


def is_local(family):
    return family_model(family).c.start_scope == _abi.SCOPE_ANYWHERE and family_model(family).c.end_scope == _abi.SCOPE_ANYWHERE


def query_is_protein(family):
    return FAMILIES[family][1] == 1


def target_is_codons(family):
    return FAMILIES[family][1] == 1 and FAMILIES[family][2] == 0


def band_rng(family, band, what=""):
    """The fixed seed of a band: the CPU proof and the device tests draw the same pairs."""
    return random.Random("edge/%s/%s/%s" % (family, band, what))


# ---- residues ---------------------------------------------------------------------------------------------------------------
# Unrelated sequence that can never lengthen an alignment: query junk and target junk share no residue (DNA: {A, C} against
# {G, T}) or score below zero against each other in every pairing and frame (protein: D / E against W / F, blosum62 -3 / -4;
# translated targets: poly-T, F in all three frames).
_HOM_AA = "ARNQGHILKMPSTYV"             # the homologous stretches leave C, D, E, F, W to the junk and the anchors


def _dna(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _qjunk(family, rng, n):
    return _dna(rng, n, "DE" if query_is_protein(family) else "AC")


def _tjunk(family, rng, n):
    if target_is_codons(family):
        return "T" * n
    return _dna(rng, n, "WF" if query_is_protein(family) else "GT")


def _other(rng, alpha, *avoid):
    return rng.choice([c for c in alpha if c not in avoid])


def _stretch(family, rng, n):
    """A homologous stretch of n query residues: (query residues, target pieces -- one per query residue), the target with a
    substitution now and then but identical over its first and last 12 residues."""
    if query_is_protein(family):
        q = [rng.choice(_HOM_AA) for _ in range(n)]
    else:
        q = [rng.choice("ACGT") for _ in range(n)]
        for k in range(1, n):                               # no residue twice in a row: a gap cannot slide along a run
            while q[k] == q[k - 1]:
                q[k] = rng.choice("ACGT")
    t = []
    for k, a in enumerate(q):
        b = a
        if 12 <= k < n - 12 and rng.random() < 0.04:
            b = _other(rng, _HOM_AA if query_is_protein(family) else "ACGT", a)
        t.append(rng.choice(CODONS[b]) if target_is_codons(family) else b)
    return q, t


def _finish(family, rng, q, t, lead=None, trail=None):
    lead = rng.randint(45, 80) if lead is None else lead         # (with the 48 residues of the shortest stretch: 128 columns and more)
    trail = rng.randint(45, 80) if trail is None else trail
    return "".join(q), _tjunk(family, rng, lead) + "".join(t) + _tjunk(family, rng, trail)


# ---- pairs of a row boundary ------------------------------------------------------------------------------------------------
# A band is (b, pad_to, full): row boundary b; every query at least pad_to residues long (unrelated residues behind the part that
# aligns: a launch takes the cooperating-wave forms from three strips per job on); full: the pair is homologous from query row 0
# on, so that b is the same row counted from the alignment's start -- else the query begins with unrelated residues up to some 60
# rows below the event, which keeps the target, and with it the oracle's work, short where only the query's own rows matter.
_NEAR = 60


def _pad(family, rng, q, pad_to):
    return q + _qjunk(family, rng, max(0, pad_to - len(q)))


def length_pairs(family, b, rng, full=True):
    """Queries of b - 2 ... b + 2 residues, homologous to their last residue: the last strip holds 0 to 3 rows beyond row 0."""
    out = []
    for qlen in range(b - 2, b + 3):
        skip = 0 if full else max(0, qlen - _NEAR)
        q, t = _stretch(family, rng, qlen - skip)
        q, t = _finish(family, rng, q, t)
        out.append({"q": _qjunk(family, rng, skip) + q, "t": t, "claims": [("start", skip), ("rows", qlen)]})
    return out


def start_pairs(family, b, rng, pad_to=0):
    """A local alignment that begins exactly at query rows b - 1, b and b + 1 behind an unrelated query prefix."""
    out = []
    for row in (b - 1, b, b + 1):
        q, t = _stretch(family, rng, 48)
        qs, ts = _finish(family, rng, q, t)
        out.append({"q": _pad(family, rng, _qjunk(family, rng, row) + qs + _qjunk(family, rng, rng.randint(0, 5)), pad_to), "t": ts,
                    "claims": [("start", row)]})
    return out


_INTRON_HEAD, _INTRON_TAIL = "GTAAGT", "TTTTCTTTTTTCAG"


def _intron(rng, n):
    """GTAAGT ... a pyrimidine tract and CAG: no other place nearby scores as a splice site."""
    n = max(n, len(_INTRON_HEAD) + len(_INTRON_TAIL) + 4)
    # (a long one is of T alone: the stretches hold no residue twice in a row, so no piece of them is worth an intron of its own)
    return _INTRON_HEAD + _dna(rng, n - len(_INTRON_HEAD) - len(_INTRON_TAIL), "ACT" if n < 1000 else "T") + _INTRON_TAIL


EVENT_KINDS = ("ins1", "ins3", "del", "ner_in", "ner_out", "intron", "intron0", "intron1", "intron2", "frameshift")


def family_events(family):
    """The event kinds a family's bands must show at its row boundaries."""
    kf = kernel_family(family)
    return {"affine": ("ins1", "ins3", "del"), "ner": ("ins1", "ins3", "del", "ner_in", "ner_out"),
            "est2genome": ("intron",), "protein2dna": ("frameshift",),
            "protein2genome": ("intron0", "intron1", "intron2")}[kf]


def event_pair(family, kind, row, rng, tail=44, intron_len=70, strand="+", lead=None, full=True, pad_to=0):
    """One pair whose oracle alignment takes an event of `kind` with its first transition starting at query row `row`: `tail`
    homologous residues behind the event (they pay for it: 44 x 5 against a gap's 12 + 4 k, an intron's 30, a frameshift's
    28), no substitution within 12 residues of it.  full: no query flank, so the alignment starts at row 0.  strand "-": the
    pair is built for the other end and both sequences are reverse-complemented (est2genome's other four states); the event still
    starts at row `row` of the query as the call sees it."""
    if strand == "-":
        # rows behind the event on the plus strand = rows in front of it on the minus strand
        fwd = event_pair(family, kind, 50, rng, tail=row if full else min(row, _NEAR), intron_len=intron_len, lead=lead)
        q = _pad(family, rng, fwd["q"], 50 + row)
        assert len(q) == 50 + row, (len(q), row)
        q = revcomp(q)
        q = _pad(family, rng, q, pad_to)                        # (unrelated residues behind the alignment, on the strand of the call)
        claims = [("event", kind, row)] + ([("start", 0)] if full else [])
        return {"q": q, "t": revcomp(fwd["t"]), "claims": claims}
    alpha = _HOM_AA if query_is_protein(family) else "ACGT"
    codons = target_is_codons(family)
    skip = 0 if full else max(0, row - _NEAR)
    at = row - skip
    n = at + tail
    q, t = _stretch(family, rng, n)
    for k in range(at - 12, at + 12):
        if 0 <= k < n:
            t[k] = CODONS[q[k]][0] if codons else q[k]
    claims = [("start", skip), ("event", kind, row)]
    if kind in ("ins1", "ins3"):
        # `extra` query residues in front of query residue `row`: the first differs from the residue behind the block and the
        # last from the residue in front of it, so the block cannot slide
        extra = 1 if kind == "ins1" else 3
        q[at:at] = [_other(rng, alpha, q[at], q[at - 1]) for _ in range(extra)]
    elif kind == "del":
        block = [_other(rng, alpha, q[at], q[at - 1]) for _ in range(rng.randint(1, 3))]
        t[at:at] = [CODONS[a][0] if codons else a for a in block]
    elif kind in ("ner_in", "ner_out"):
        # unrelated residues on both sides between two anchors: the ner state is entered with the first of them.  ner_out: the
        # block's last query residue is residue row - 1, so "ner to match" is taken in row `row`
        x, y = rng.randint(9, 14), rng.randint(9, 14)
        where = at if kind == "ner_in" else at - x
        q[where:where] = list(_qjunk(family, rng, x))
        t[where:where] = list(_tjunk(family, rng, y))
    elif kind == "frameshift":
        q[at - 1:at + 1] = "WW"                          # TGG C TGG: no other cut of these bases reads W twice
        t[at - 1:at + 1] = ["TGG", "TGG"]
        t[at:at] = ["C" * rng.randint(1, 2)]
    elif kind == "intron":
        t[at:at] = [_intron(rng, intron_len)]
        q[at - 3:at + 1] = list("CAGG")                  # ... CAG | GTAAGT ... CAG | G ...: the consensus exon ends
        t[at - 3:at] = list("CAG")
        t[at + 1] = "G"
    elif kind in ("intron0", "intron1", "intron2"):
        phase = int(kind[-1])
        if phase == 0:
            t[at:at] = [_intron(rng, intron_len)]
        else:
            c = t[at]
            t[at] = c[:phase] + _intron(rng, intron_len) + c[phase:]
    else:
        raise ValueError(kind)
    qs, ts = _finish(family, rng, q, t, lead)
    return {"q": _pad(family, rng, _qjunk(family, rng, skip) + qs, pad_to), "t": ts, "claims": claims}


def event_pairs(family, b, rng, full=True, pad_to=0):
    """Each event of the family with its transition starting at row b - 1 and, in another pair, at row b (an insertion of three
    also at b - 2: opened below the edge, extended across it; introns also on row b + 1), est2genome on both strands."""
    out = []
    for kind in family_events(family):
        rows = (b - 2, b - 1, b) if kind == "ins3" else (b - 1, b, b + 1) if kind.startswith("intron") else (b - 1, b)
        for row in rows:
            out.append(event_pair(family, kind, row, rng, full=full, pad_to=pad_to))
            if kind == "intron":
                out.append(event_pair(family, kind, row, rng, strand="-", full=full, pad_to=pad_to))
    return out


def tie_pairs(family, b, rng, pad_to=0):
    """Ties that are decided across structure (local models): a motif twice in the query -- below row b / 2 and above row b --
    against a target that holds it once (two end cells in different strips, waves or super-strips), the transpose (two end
    cells in different columns: chunks, windows), and for the DNA families with affine gaps a gap of three that may be taken on
    either axis first, next to the edge (parameter point "cheap").  ner joins chance matches between a motif and the other
    side's unrelated residues through its free loops, so its motif is of C and G alone between A's in the query and T's in the
    target: nothing but the motif's own copies can match."""
    unit = 3 if target_is_codons(family) else 1
    if kernel_family(family) == "ner":
        motif = list(_dna(rng, 30, "CG"))
        mt = list(motif)
        qj = lambda n: "A" * n
        tj = lambda n: "T" * n
    else:
        motif, mt = _stretch(family, rng, 30)
        mt = [CODONS[a][0] if target_is_codons(family) else a for a in motif]
        qj = lambda n: _qjunk(family, rng, n)
        tj = lambda n: _tjunk(family, rng, n)
    first = max(2, b // 2 - 30)
    gap = b + 3 - first - 30
    q = qj(first) + "".join(motif) + qj(gap) + "".join(motif) + qj(max(7, pad_to - first - gap - 60))
    t = tj(33) + "".join(mt) + tj(40)
    out = [{"q": q, "t": t, "claims": [("tie_rows", first + 30, first + 30 + gap)]}]
    q = qj(b - 28) + "".join(motif) + qj(max(9, pad_to - b - 2))                          # the motif ends on row b + 2
    lead, between = 41 * unit, 70 * unit                       # (copies in different 64-column chunks)
    t = tj(lead) + "".join(mt) + tj(between) + "".join(mt) + tj(20)
    out.append({"q": q, "t": t, "claims": [("tie_cols", lead + 30 * unit, lead + 30 * unit + between)]})
    if kernel_family(family) in ("affine", "est2genome") and not query_is_protein(family):
        # ... C AAA G ... against ... C TTT G ...: three query residues and three target residues that match nothing, at a point
        # where two gaps of three (2 x -4) cost less than three mismatches (-12).  "Insertion, then deletion" and "deletion, then
        # insertion" visit the same matches and pay the same two gaps, so they tie by construction and the transition order decides;
        # the claim is that the oracle takes one gap on each axis there.  Two pairs (rows b - 1 and b), so the call of this
        # parameter point has two jobs, as the packed forms ask.
        for row in (b - 1, b):
            skip = max(0, row - _NEAR)
            h, ht = _stretch(family, rng, row - skip + 41)
            at = row - skip
            h[at - 1:at + 1] = "CG"                          # neither block can slide
            for k in range(at - 13, at + 15):
                ht[k] = h[k]
            qs = _qjunk(family, rng, skip) + "".join(h[:at]) + "AAA" + "".join(h[at:])
            ts = "".join(ht[:at]) + "TTT" + "".join(ht[at:])
            out.append({"q": _pad(family, rng, qs, pad_to), "t": _tjunk(family, rng, 25) + ts + _tjunk(family, rng, 25),
                        "point": "cheap", "claims": [("start", skip), ("gap_both_axes", row)]})
    return out


def band_of(b, pad_to=0, full=None):
    """The band key of row boundary b; full defaults to b <= 384 (the strips of the path, checkpoint and continuation kernels,
    which count from the alignment's start, are at most that high)."""
    return (b, pad_to, (b <= 384) if full is None else full)


def row_band(family, band):
    """Every pair of a band (b, pad_to, full), one batch."""
    b, pad_to, full = band
    full = full or not is_local(family)                    # (a model that is not local aligns the unrelated residues too)
    rng = band_rng(family, band)
    out = length_pairs(family, b, rng, full) if b - 2 >= pad_to else []
    if is_local(family):
        out += start_pairs(family, b, rng, pad_to) + tie_pairs(family, b, rng, pad_to)
    out += event_pairs(family, b, rng, full, pad_to)
    return out


# ---- pairs of the column boundaries -----------------------------------------------------------------------------------------
def col_band(family, rows, cols=COL_BANDS, long_intron=False, longest=0):
    """One batch for the column boundaries `cols` (target columns; for the translated targets the same numbers are nucleotide
    columns), every query `rows` ... `rows` + 40 residues long so that the launch takes the cooperating-wave forms: targets
    of c - 1, c and c + 1 columns, alignments that end at columns c - 1, c and c + 1 with junk behind them, and for the families
    with introns one that begins at column c - 1 and one that ends at c + 1 (with a dump every 32 or 64 columns they start on and
    jump over a dump column; at c = 64 the intron that ends at c + 1 is 32 columns long behind 10 or 14 query rows, the others 70
    behind 14).  long_intron: one more pair with an intron longer than 32 767 columns.  longest: the first pair's query carries
    unrelated residues up to that length -- the longest query of a launch decides the form of the packed score pass, so one long
    query puts the whole band on the six-row or the long form."""
    rng = band_rng(family, "cols", rows)
    unit = 3 if target_is_codons(family) else 1
    introns = kernel_family(family) in ("est2genome", "protein2genome")
    local_only = lambda *claims: list(claims) if is_local(family) else []      # (the other scopes end where the sequences do)
    out = []
    for c in cols:
        for tlen in (c - 1, c, c + 1):
            # the target is homologous to the query's end up to its own last column
            n = min(tlen // unit, 50)
            h, ht = _stretch(family, rng, n)
            lead = tlen - n * unit
            q = _qjunk(family, rng, rows + rng.randint(0, 40) - n) + "".join(h)
            out.append({"q": q, "t": _tjunk(family, rng, lead) + "".join(ht), "claims": [("cols", tlen)] + local_only(("end_col", tlen))})
        for end in (c - 1, c, c + 1):
            n = min(end // unit, 40)
            h, ht = _stretch(family, rng, n)
            lead = end - n * unit
            at = rng.randint(0, rows - n)
            q = _qjunk(family, rng, at) + "".join(h) + _qjunk(family, rng, rows + rng.randint(0, 40) - at - n)
            out.append({"q": q, "t": _tjunk(family, rng, lead) + "".join(ht) + _tjunk(family, rng, 45 * unit),
                        "claims": local_only(("end_col", end))})
        if introns:
            kind = "intron" if kernel_family(family) == "est2genome" else "intron0"
            for where in ("from", "to"):
                ilen, row = (70, 14) if c >= 128 or where == "from" else (32, 14 if unit == 1 else 10)
                lead = c - 1 - row * unit if where == "from" else c + 1 - ilen - row * unit
                pair = event_pair(family, kind, row, rng, intron_len=ilen, lead=lead, pad_to=rows + rng.randint(0, 40))
                pair["claims"] = [("intron_from", c - 1) if where == "from" else ("intron_to", c + 1), ("intron_over", c)]
                out.append(pair)
    if long_intron:
        pair = event_pair(family, "intron", 40, rng, intron_len=33000 + rng.randint(0, 400), pad_to=rows)
        pair["claims"] = [("intron_longer", 32767)]
        out.append(pair)
    if longest:
        n = next(n for n, p in enumerate(out) if len(p["t"]) >= 256)       # (a pair that every dump interval in use windows)
        out[n] = dict(out[n], q=_pad(family, rng, out[n]["q"], longest))
    return out


def small_band(family):
    """Lengths 0, 1, 2 and 3 on either side -- for the translated targets 0 ... 5 nucleotides, so fewer columns than the largest
    target advance, in all three frames -- and an empty query beside a non-empty one: one batch."""
    rng = band_rng(family, "small")
    prot, codons = query_is_protein(family), target_is_codons(family)
    word = [rng.choice("WCM") if prot else "ACGT"[k] for k in range(3)]
    tword = "".join(CODONS[a][0] if codons else a for a in word)
    out = []
    for qlen in range(4):
        for tlen in range(6 if codons else 4):
            for frame in (range(3) if codons and tlen >= 3 else (0,)):
                t = ("T" * frame + tword)[:tlen] if codons else tword[:tlen]
                out.append({"q": "".join(word[:qlen]), "t": t, "claims": []})
    out.append({"q": "".join(word), "t": _tjunk(family, rng, 4) + tword + tword, "claims": []})
    return out


# ---- what an alignment shows ------------------------------------------------------------------------------------------------
def events(model, aln):
    """The events of alignment dict `aln` in path order: dicts {"kind", "row", "col", "end_col", "length"}; row and col are the
    cell in which the event's first transition starts.  Kinds: ins (query residues against nothing), del, ner, intron (with
    "phase": the nucleotides of a split codon in front of it, and "label": the first splice site's), frameshift."""
    if aln is None:
        return []
    m = model.c
    i, j = aln["region"][0], aln["region"][1]
    out, cur, phase, phase_cell = [], None, 0, None
    for tr, length in aln["ops"]:
        t = m.transitions[tr]
        name = bytes(t.name).split(b"\0")[0].decode()
        for _ in range(length):
            kind = None
            if t.label == _abi.LABEL_GAP:
                kind = "ins" if t.advance_query else "del"
            elif t.label == _abi.LABEL_NER:
                kind = "ner"
            elif t.label == _abi.LABEL_FRAMESHIFT:
                kind = "frameshift"
            elif t.label in (_abi.LABEL_5SS, _abi.LABEL_3SS, _abi.LABEL_INTRON):
                kind = "intron"
            elif t.label == _abi.LABEL_SPLIT_CODON and t.advance_query == 0:
                phase, phase_cell = t.advance_target, (i, j)
            if kind is not None and cur is not None and cur["kind"] == kind and not cur.get("closed"):
                cur["length"] += 1
                cur["end_col"] = j + t.advance_target
                if kind == "intron" and t.label in (_abi.LABEL_5SS, _abi.LABEL_3SS):
                    cur["closed"] = True
            elif kind is not None:
                cur = {"kind": kind, "row": i, "col": j, "end_col": j + t.advance_target, "length": 1}
                if kind == "intron":
                    cur["phase"], cur["label"] = phase, t.label
                    phase = 0
                out.append(cur)
            elif t.advance_query or t.advance_target or name == "ner to match":
                if cur is not None and cur["kind"] == "ner" and name == "ner to match":
                    cur["out_row"] = i
                cur = None
            i += t.advance_query
            j += t.advance_target
    return out


def event_rows(model, aln):
    """{(kind of EVENT_KINDS, query row at which its first transition starts)} of an alignment."""
    seen = set()
    for e in events(model, aln):
        if e["kind"] == "ins":
            seen.add(("ins1" if e["length"] == 1 else "ins3" if e["length"] >= 3 else "ins2", e["row"]))
        elif e["kind"] == "ner":
            seen.add(("ner_in", e["row"]))
            if "out_row" in e:
                seen.add(("ner_out", e["out_row"]))
        elif e["kind"] == "intron":
            seen.add(("intron", e["row"]))
            seen.add(("intron%d" % e["phase"], e["row"]))
        else:
            seen.add((e["kind"], e["row"]))
    return seen


def _score(model, q, t):
    return oracle_lib.find_score(model.c, model.params, q.encode(), t.encode())


def pair_shows(model, pair, aln):
    """None where the oracle's alignment `aln` (dict) of `pair` shows every claim the pair makes, else what is missing."""
    if aln is None:
        return "no alignment"
    q, t = pair["q"], pair["t"]
    rows = None
    for claim in pair["claims"]:
        what = claim[0]
        if what == "event":
            rows = event_rows(model, aln) if rows is None else rows
            ok = (claim[1], claim[2]) in rows
        elif what == "start":
            ok = aln["region"][0] == claim[1]
        elif what == "rows":
            ok = len(q) == claim[1] and aln["region"][0] + aln["region"][2] == claim[1]
        elif what == "cols":
            ok = len(t) == claim[1]
        elif what == "end_col":
            ok = aln["region"][1] + aln["region"][3] == claim[1]
        elif what in ("intron_from", "intron_to", "intron_over", "intron_longer"):
            introns = [e for e in events(model, aln) if e["kind"] == "intron"]
            ok = any({"intron_from": e["col"] == claim[1], "intron_to": e["end_col"] == claim[1],
                      "intron_over": e["col"] < claim[1] < e["end_col"],
                      "intron_longer": e["end_col"] - e["col"] > claim[1]}[what] for e in introns)
        elif what == "gap_both_axes":
            ev = [e for e in events(model, aln) if e["kind"] in ("ins", "del") and e["row"] in (claim[1], claim[1] + 3)]
            ok = {e["kind"] for e in ev} == {"ins", "del"} and all(e["length"] == 3 for e in ev)
        elif what == "tie_rows":
            whole = _score(model, q, t)
            ok = whole > 0 and _score(model, q[:claim[1]], t) == whole == _score(model, q[claim[2]:], t)
        elif what == "tie_cols":
            whole = _score(model, q, t)
            ok = whole > 0 and _score(model, q, t[:claim[1]]) == whole == _score(model, q, t[claim[2]:])
        else:
            raise ValueError(claim)
        if not ok:
            return "%r does not hold: region %r, events %r" % (claim, aln["region"], sorted(event_rows(model, aln)))
    return None


# ---- the oracle's answers, computed once per band and shared by every test of the process --------------------------------------
_ORACLE = {}


def band_pairs(family, band):
    """band: a row band (b, pad_to, full) -- see band_of --, ("cols", rows[, longest]), ("cols+long", rows[, longest]) -- see
    col_band --, "small", or ("c8", any of these):
    that band with the ambiguity codes N, R and Y in front of every target (seven residue codes in the batch)."""
    key = (family, band, "pairs")
    if key not in _ORACLE:
        if band == "small":
            _ORACLE[key] = small_band(family)
        elif band[0] == "c8":
            _ORACLE[key] = [dict(p, t="NRY" + p["t"][3:]) for p in band_pairs(family, band[1])]
        elif isinstance(band[0], str):
            _ORACLE[key] = col_band(family, band[1], long_intron=band[0] == "cols+long", longest=band[2] if len(band) > 2 else 0)
        else:
            _ORACLE[key] = row_band(family, band)
    return _ORACLE[key]


def pair_model(family, pair):
    return family_model(family, pair.get("point", "default"))


def oracle_paths(family, band, dpm):
    """The oracle's find_path (alignment dicts, None where there is none) of the band's pairs at dpmemory `dpm`."""
    key = (family, band, dpm)
    if key not in _ORACLE:
        out = []
        for p in band_pairs(family, band):
            one = (family, p.get("point", "default"), p["q"], p["t"], dpm)       # (bands share pairs: the column band's variants)
            if one not in _ORACLE:
                m = pair_model(family, p)
                _ORACLE[one] = oracle_lib.find_path(m.c, m.params, p["q"].encode(), p["t"].encode(), dpmemory=dpm)
            out.append(_ORACLE[one])
        _ORACLE[key] = out
    return _ORACLE[key]


def oracle_scores(family, band):
    key = (family, band, "score")
    if key not in _ORACLE:
        _ORACLE[key] = [_score(pair_model(family, p), p["q"], p["t"]) for p in band_pairs(family, band)]
    return _ORACLE[key]


def band_shows(family, band):
    """None, or the first claim of the band that the oracle's alignments (dpmemory 32) do not show.  Besides each pair's own
    claims, a row band must show -- over its pairs -- every event kind of the family starting at row b - 1 and at row b, a
    transition from row b - 1 to row b counted from the query's first row and from the alignment's, queries of b - 2 ... b + 2
    residues and, for the local models, alignments that start at rows b - 1, b and b + 1."""
    pairs, alns = band_pairs(family, band), oracle_paths(family, band, 32)
    for n, (p, a) in enumerate(zip(pairs, alns)):
        if a is None and band != "small":
            return "pair %d: no alignment" % n
        if a is not None:
            miss = pair_shows(pair_model(family, p), p, a)
            if miss:
                return "pair %d (%d x %d): %s" % (n, len(p["q"]), len(p["t"]), miss)
    if band != "small" and band[0] == "c8":
        band = band[1]                   # (the claims of the band inside were checked above on the pairs with the codes in front)
    if band == "small" or isinstance(band[0], str):
        return None
    b, pad_to, full = band
    full = full or not is_local(family)
    seen = set().union(*[event_rows(pair_model(family, p), a) for p, a in zip(pairs, alns)])
    for kind in family_events(family):
        for row in (b - 1, b):
            if (kind, row) not in seen:
                return "no %s starting at row %d" % (kind, row)
    for origin in ((False, True) if full else (False,)):
        if not any(crossings(pair_model(family, p), a, b, origin) for p, a in zip(pairs, alns)):
            return "no transition across row %d (rows of the %s)" % (b, "region" if origin else "query")
    if b - 2 >= pad_to and not {len(p["q"]) for p in pairs} >= set(range(b - 2, b + 3)):
        return "no queries of %d ... %d residues" % (b - 2, b + 2)
    if is_local(family) and not {b - 1, b, b + 1} <= {a["region"][0] for a in alns}:
        return "no alignment starting at rows %d ... %d" % (b - 1, b + 1)
    return None


# ---- forms: the switches of one case of the device tests, the launches they lead to, and where those cut the rectangle ----------
def form_boundaries(geometries):
    """{row boundary: what it is} of a form, from the geometry dicts (kernel_choice_sim_lib.geometry / form_geometry) of the
    kernels its launches take: each kernel's strip height 64 R and workgroup height waves x 64 R; for a staged packed score
    kernel (name kpk16e ... kpk16j) the rows one workgroup stages -- staged_rows, staged_rows6 for the six-row forms, which is
    also the super-strip of the long form."""
    out = {}
    for g in geometries:
        if not g["name"]:
            continue
        strip = 64 * g["R"]
        out.setdefault(strip, "strip of " + g["name"])
        # (hbm_carry: cooperating waves whose strip carry rows go through the workgroup's slab in HBM, not through LDS rings)
        out.setdefault(strip * g["waves"], "workgroup of " + g["name"] + (" (carry rows through HBM)" if g["hbm_carry"] and g["waves"] > 1 else ""))
        stem = g["name"].split("_")[0]
        if stem in ("kpk16e", "kpk16f", "kpk16g", "kpk16i"):
            out.setdefault(g["staged_rows"], "staged rows of " + g["name"])
        if stem in ("kpk16h", "kpk16j"):
            out.setdefault(g["staged_rows6"], ("super-strip of " if stem == "kpk16j" else "staged rows of ") + g["name"])
    return out


def form_bands(geometries, bands=ROW_BANDS):
    """The bands of ROW_BANDS that fall on a row boundary of the form, ascending."""
    at = form_boundaries(geometries)
    return [b for b in bands if b in at]


# The 32-bit forms: name -> (C4GPU_* switches of the case, the passes whose kernels the form is about -- their boundaries are the
# form's bands).  Every case runs find_score and find_path at dpmemory 32 and 0, so all five passes run in each.
PASSES = ("score", "region", "path", "ckpt_cont", "path_cont")
FORMS32 = {
    "one-wave": ({"MW": "0"}, PASSES),
    "four-waves": ({"MW": "4"}, ("score", "region")),
    "eight-waves": ({}, ("score", "region")),
    "general": ({"LOCAL_EXACT": "0"}, ("score", "region")),
    "two-slot": ({"PACK": "0"}, ("region",)),
    "cont-masks": ({"CONT_FREE": "0"}, ("ckpt_cont", "path_cont")),
    "host-route": ({"FUSED": "0"}, ("ckpt_cont", "path_cont")),
    "device-route": ({"FUSED": "1"}, ("ckpt_cont", "path_cont")),
}
CU_COUNT = 256


def launch_facts(family, env, what, **more):
    """The LaunchFacts (kernel_choice_sim_lib.FACTS) of pass `what` of a call on `family` under the switches `env`, as
    Engine::run_impl fills them for a batch whose region starts fit the packed slot."""
    import kernel_choice_sim_lib as kc
    local = is_local(family)
    f = dict(family=kc.FAMILY[kernel_family(family)], local=int(local), local_exact=int(local and env.get("LOCAL_EXACT") != "0"),
             cu_count=CU_COUNT)
    f["mode"] = {"score": kc.SCORE, "region": kc.REGION, "path": kc.PATH, "ckpt_cont": kc.CKPT, "path_cont": kc.PATH}[what]
    if what == "region":
        f["starts_pack"] = 1
    if what.endswith("_cont"):
        f["cont"], f["cont_free"] = 1, int(env.get("CONT_FREE") != "0")
    f.update(more)
    return f


def shim_switches(env):
    import kernel_choice_sim_lib as kc
    return {k: int(v) for k, v in env.items() if k in kc.SWITCHES}


def form_launches(family, form, query_lengths):
    """{pass: geometry of the kernel that serves it} for a batch of these query lengths under a form of FORMS32."""
    import kernel_choice_sim_lib as kc
    env = FORMS32[form][0]
    return {what: kc.geometry(list(query_lengths), shim_switches(env), **launch_facts(family, env, what)) for what in PASSES}


def form32_bands(family, form):
    """The bands (band_of keys) of a 32-bit form: the ROW_BANDS on a strip or workgroup edge of the kernels the form is about,
    with queries padded to 520 residues where a launch of the form takes cooperating waves (three strips of 64 x 4 rows per
    job); [] where the table does not hold the form for this family (the switches lead to the kernels of another form)."""
    nominal = [800] * 24
    got = form_launches(family, form, nominal)
    default = form_launches(family, "eight-waves", nominal)
    held = {"one-wave": True,
            "four-waves": got["score"]["waves"] == 4, "eight-waves": got["score"]["waves"] == 8,
            "general": "_local" not in got["score"]["name"] and got["score"]["name"] != default["score"]["name"],
            "two-slot": "_pack" not in got["region"]["name"],
            "cont-masks": "_local" not in got["ckpt_cont"]["name"],
            "host-route": True, "device-route": True}[form]
    if not held:
        return []
    mw = got["score"]["waves"] > 1 or got["region"]["waves"] > 1
    return [band_of(b, 520 if mw else 0) for b in form_bands([got[w] for w in FORMS32[form][1]])]


# ---- the seeded (windowed) and packed forms ------------------------------------------------------------------------------------
# name -> (family, switches, which launches the form is about: "seed1" the score pass with dumps, "seed2" the region windows,
# "ck16" the packed checkpoint pass).  A dump every 32 columns: find_path_batch windows every pair with T >= 128.
KSHIFT = 5
_PACKED = {"SEED_KSHIFT": str(KSHIFT), "PK16_NW8": "0"}
FORMS_SEEDED = {
    "win32/est2genome/nw2": ("est2genome", {"SEED_KSHIFT": "5", "PK16": "0", "CK16": "0", "WIN_NW": "2"}, ("seed1", "seed2")),
    "win32/est2genome/nw4": ("est2genome", {"SEED_KSHIFT": "5", "PK16": "0", "CK16": "0", "WIN_NW": "4"}, ("seed1", "seed2")),
    "win32/est2genome/mw4": ("est2genome", {"SEED_KSHIFT": "6", "PK16": "0", "CK16": "0", "MW": "4"}, ("seed1",)),
    "win32/protein2genome": ("protein2genome", {"SEED_KSHIFT": "5"}, ("seed1", "seed2")),
    "win32/protein2genome/mw4": ("protein2genome", {"SEED_KSHIFT": "6", "MW": "4"}, ("seed1",)),
    # (C4GPU_PK16=1 EXACTLY puts the forms with 16-bit dumps behind PK16_PLAIN -- the io cases below --, so PK16_PLAIN itself, with its
    # 32-bit dumps, is asked for with 2: c4_kernel_choice.h, Switches::pk16)
    "pk16/plain": ("est2genome", dict(_PACKED, PK16="2"), ("seed1",)),
    "pk16/asm": ("est2genome", dict(_PACKED, PK16="3"), ("seed1",)),
    "pk16/counters": ("est2genome", dict(_PACKED, PK16="4"), ("seed1",)),
    "pk16/io0": ("est2genome", dict(_PACKED, PK16_IO="0"), ("seed1",)),
    "pk16/io1": ("est2genome", dict(_PACKED, PK16_IO="1"), ("seed1",)),
    "pk16/io2": ("est2genome", dict(_PACKED, PK16_IO="2"), ("seed1",)),
    "pk16/nw8": ("est2genome", dict(_PACKED, PK16_NW8="1"), ("seed1",)),
    "pk16/r6": ("est2genome", dict(_PACKED, PK16_R6="1"), ("seed1",)),
    "pk16/long": ("est2genome", dict(_PACKED, PK16_R6="1", PK16_LONG="1"), ("seed1",)),
    "pk16/c8": ("est2genome", dict(_PACKED), ("seed1",)),
}
for _k in range(2, 11):
    FORMS_SEEDED["win16/%d" % _k] = ("est2genome", dict(_PACKED, WIN16=str(_k)), ("seed2",))
for _k in range(2, 10):
    FORMS_SEEDED["ck16/%d" % _k] = ("est2genome", dict(_PACKED, CK16=str(_k)), ("ck16",))
FORMS_SEEDED["ck16/unrooted"] = ("est2genome", dict(_PACKED, CK16_ROOT="0"), ("ck16",))


def seeded_geometry(form, query_lengths, tdense_n=5):
    """{"seed1" / "seed2" / "ck16": geometry} of the launches a form of FORMS_SEEDED is about, for a windowed batch of these
    query lengths (est2genome: all of them fit the packed pass)."""
    family, env, about = FORMS_SEEDED[form]
    return launches_seeded(family, env, about, query_lengths, tdense_n)


def launches_seeded(family, env, about, query_lengths, tdense_n=5):
    """The same for any switches: `about` names the launches wanted ("ck16" needs C4GPU_CK16 pinned to a shape, or
    C4GPU_CK16_ROOT=0: by default the rooted shape follows the regions the score pass found)."""
    import kernel_choice_sim_lib as kc
    sw = shim_switches(env)
    kshift = int(env["SEED_KSHIFT"])
    packed = family == "est2genome" and env.get("PK16") != "0"
    out = {}
    base = dict(pk16_params_ok=int(family == "est2genome"), tdense_n=tdense_n, kshift=kshift)
    one = kc.geometry(list(query_lengths), sw, **launch_facts(family, env, "score", seed_mode=1, pk16_all_fit=int(packed), **base))
    if "seed1" in about:
        out["seed1"] = one
    if "seed2" in about:
        fmt16 = int(packed and one["name"] is not None and one["name"].split("_")[0] in
                    ("kpk16d", "kpk16e", "kpk16f", "kpk16g", "kpk16h", "kpk16i", "kpk16j"))
        out["seed2"] = kc.geometry(list(query_lengths), sw, **launch_facts(family, env, "region", seed_mode=2, fmt16=fmt16,
                                                                           ss16_built=fmt16, **base))
    if "ck16" in about:
        if env.get("CK16_ROOT") == "0":
            out["ck16"] = kc.form_geometry(kc.CK16, family, 0)
        else:
            k = int(env["CK16"])
            out["ck16"] = kc.form_geometry(kc.CK16_ROOTED, family, 0 if k == 8 else k - 1)
    return out


def seeded_bands(form):
    """The bands of a seeded or packed form: the ROW_BANDS on a strip, workgroup, staged-rows or super-strip edge of the kernels
    the form is about, every query at least 520 rows (the windows' domain and three strips per job) -- at least staged_rows + 6
    (staged_rows6 + 6) for the six-row (long) form, which the longest query of a launch selects (at the six-row form's own
    workgroup edge the band runs in two calls: seeded_calls); the packed checkpoint pass counts rows from the alignment's start,
    so its bands are homologous from row 0 on."""
    family, env, about = FORMS_SEEDED[form]
    nominal = {"pk16/r6": 1100, "pk16/long": 1600}.get(form, 800)
    geo = seeded_geometry(form, [nominal] * 24, 7 if form == "pk16/c8" else 5)
    bands = form_bands([geo[w] for w in about])
    if form == "pk16/r6":
        bands = sorted(set(bands) | {geo["seed1"]["staged_rows"]})       # ... and the row at which the choice turns to it
    pad = {"pk16/r6": geo.get("seed1", {}).get("staged_rows", 0) + 6, "pk16/long": geo.get("seed1", {}).get("staged_rows6", 0) + 6}
    out = []
    for b in bands:
        band = band_of(b, pad.get(form, 520), True if "ck16" in about else None)
        out.append(("c8", band) if form == "pk16/c8" else band)
    return out


STAGED_ONE_WORKGROUP = ("pk16/io1", "pk16/io2", "pk16/nw8", "pk16/c8")


def seeded_calls(form, band):
    """The band's pairs by the call they run in: [[index of each pair]].  One call -- but at the band of the rows their
    workgroup stages (staged_rows; the six-row form: staged_rows6) the staged forms take two: the longest query of a launch
    decides its kernel, so the queries that fit the staged rows run by themselves (the form under test) and the longer ones
    beside them (the form the choice then turns to)."""
    family = FORMS_SEEDED[form][0]
    pairs = band_pairs(family, band)
    everything = list(range(len(pairs)))
    if band == "small" or (isinstance(band[0], str) and band[0] != "c8") or form not in STAGED_ONE_WORKGROUP + ("pk16/r6",):
        return [everything]
    row = (band[1] if band[0] == "c8" else band)[0]
    geo = seeded_geometry(form, [800] * 24)["seed1"]
    staged = geo["staged_rows6"] if form == "pk16/r6" else geo["staged_rows"]
    if row != staged:
        return [everything]
    return [[n for n in everything if len(pairs[n]["q"]) + 1 <= staged], [n for n in everything if len(pairs[n]["q"]) + 1 > staged]]


def seeded_col_band(form):
    """The column band a seeded or packed form runs: 530-row queries (the windows' domain); for the packed forms with the intron
    longer than the 15-bit length counter; for the six-row and the long form with one query long enough to select them."""
    family, env, about = FORMS_SEEDED[form]
    packed = family == "est2genome" and env.get("PK16") != "0"
    geo = seeded_geometry(form, [800] * 24).get("seed1", {})
    longest = {"pk16/r6": geo.get("staged_rows", 0) + 6, "pk16/long": geo.get("staged_rows6", 0) + 6}.get(form, 0)
    band = ("cols+long" if packed else "cols", 530) + ((longest,) if longest else ())
    return ("c8", band) if form == "pk16/c8" else band
