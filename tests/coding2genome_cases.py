"""The vector sets of coding2genome (src/model/coding2genome.c:53-74: coding2coding plus the phase model against DNA, target
introns in phase 0, 1:2 and 2:1 with split codons either side), their loaders, the replay of a recorded path through the model's
tables and the generators of the pairs the device tests make on the spot (data and plumbing only; no reference code).  The sets
are made by tools/make_coding2genome_golden.py from the reference itself (refdump, the reference binary):
  * coding2genome.jsonl (-D 32; with the splice values at the sites its paths use, rec["ss"]), coding2genome_D0.jsonl (-D 0),
    coding2genome_alt.jsonl (rec["point"]: golden_util's altparams or tightintron), coding2genome_subopt.jsonl (the GAM loop);
  * codon_cli_coding2genome.json: stdout of `exonerate --model coding2genome --exhaustive yes`, one run per pair, one of them
    with its best alignment on the target's minus strand.
No test routes this model through the CPU oracle (its split-codon calc is the protein query's): the yardstick is the reference."""
import json, os, random

import exonerate_amd as ex
from exonerate_amd import _abi
from golden_util import GOLDEN_DIR, PARAM_VARIANTS, apply_flags, load_set

# set -> dpmemory
SETS = {"coding2genome": 32, "coding2genome_D0": 0, "coding2genome_alt": 32}
SUBOPT_SET = "coding2genome_subopt"
SUBOPT_FLAGS = ["--suboptmax", "4", "--suboptthreshold", "30"]
SUBOPT_MAX = 4
CLI_SET = "codon_cli_coding2genome"
CLI_REPORTS = ["--showalignment", "yes", "--showvulgar", "yes", "--showtargetgff", "yes"]
POINT_FLAGS = {"default": [], "altparams": PARAM_VARIANTS["altparams"], "tightintron": PARAM_VARIANTS["tightintron"],
               # an intron, a frameshift and a codon gap each cost less than two matched codons score
               "cheap": ["--intronpenalty", "-12", "--frameshift", "-9", "--codongapopen", "-9", "--codongapextend", "-2"]}
AA = "ARNDCQEGHILKMFPSTWYV"
_NCBI = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODONS = {}
for _i, _a in enumerate("TCAG"):
    for _j, _b in enumerate("TCAG"):
        for _k, _c in enumerate("TCAG"):
            CODONS.setdefault(_NCBI[_i * 16 + _j * 4 + _k], []).append(_a + _b + _c)
_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def point_model(point):
    return ex.Model("coding2genome", params=apply_flags(ex.default_params(), POINT_FLAGS[point]))


def rec_model(rec):
    return point_model(rec.get("point", "default"))


def load_cli():
    with open(os.path.join(GOLDEN_DIR, CLI_SET + ".json")) as f:
        return json.load(f)


# ---- the recorded path through the tables ------------------------------------------------------------------------------
def codon_code(params, bases):
    a, b, c = (params.nt2d[ord(x)] for x in bases)
    return params.submat_index[params.aa[params.trans[a | (b << 4) | (c << 8)]]]


def introns_of(model, ops, region):
    """[(phase, target start, length)] of the introns of a path: phase 0, 1 or 2 by the intron state's name ("intron 1:2 ...")."""
    m = model.c
    j, out, start = region[1], [], None
    for tr, length in ops:
        t = m.transitions[tr]
        if t.label == _abi.LABEL_5SS:
            start = j
        j += t.advance_target * length
        if t.label == _abi.LABEL_3SS:
            out.append((int(m.state_names[t.input].value.decode().split()[1][0]), start, j - start))
    return out


def replay(model, rec, ops=None, region=None):
    """Walks the ops through the model's transition table, asserting that they chain from START to END: (score or None, query
    advance, target advance, labels seen).  The score is added up where the record carries the splice values of the sites its path
    uses (rec["ss"] = {"5": {position: value}, "3": {...}}): the codon match is protein_submat[aa(q[i..i+2])][aa(t[j..j+2])]
    (match.c:508-530), a 5' site the intron penalty plus its value and a 3' site its value, both read at the transition's first
    target position (intron.c:150-160), and a split codon the same matrix on the query's three bases in front of the transition's
    end and the target's codon re-assembled across the intron (phase.c:139-208)."""
    m, p = model.c, model.params
    ops = rec["ops"] if ops is None else ops
    region = rec["region"] if region is None else region
    q, t = rec["query"], rec["target"]
    ss = rec.get("ss")
    i, j, score, state, labels, shadow = region[0], region[1], 0, m.start_state, set(), None
    for tr, length in ops:
        d = m.transitions[tr]
        for _ in range(length):
            assert d.input == state, (rec["id"], tr, state)
            if d.calc >= 0:
                c = m.calcs[d.calc]
                if c.kind == _abi.CALC_MATCH_CODON:
                    score += p.protein_submat[codon_code(p, q[i:i + 3])][codon_code(p, t[j:j + 3])]
                elif c.kind == _abi.CALC_CONST:
                    score += c.value
                elif c.kind == _abi.CALC_SPLICE_PRE:
                    shadow = j
                    if ss is not None:
                        score += c.value + ss["5"][str(j)]
                elif c.kind == _abi.CALC_SPLICE_POST:
                    length_ = j + 2 - shadow
                    assert p.min_intron <= length_ <= p.max_intron, (rec["id"], length_)
                    if ss is not None:
                        score += ss["3"][str(j)]
                else:
                    assert c.kind == _abi.CALC_PHASE_POST and shadow is not None
                    iq = i + d.advance_query - 3
                    assert iq >= 0 and shadow >= c.param, rec["id"]
                    tb = t[shadow - 1] + t[j:j + 2] if c.param == 1 else t[shadow - 2:shadow] + t[j]
                    score += p.protein_submat[codon_code(p, q[iq:iq + 3])][codon_code(p, tb)]
            i += d.advance_query
            j += d.advance_target
            state = d.output
            labels.add(d.label)
    assert state == m.end_state, rec["id"]
    return (score if ss is not None else None), i - region[0], j - region[1], labels


# ---- generated pairs ---------------------------------------------------------------------------------------------------
def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def intron(rng, n):
    """n bases GT ... AG: a 5' site near the consensus, a pyrimidine tract in front of the 3' site, no AG inside the tract."""
    assert n >= 20
    return "GTAAGT" + "".join(rng.choice("ACT") for _ in range(n - 18)) + "TTTCTTTTTCAG"


def gene_pair(rng, n_aa, introns=(), events=(), flank_q=0, flank_t=None, sub=0.06, keep=3):
    """A CDS of n_aa codons and its gene: the same peptide in other synonymous codons (`sub` of the residues replaced), with
    introns = [(codon, phase, length)] put `phase` bases into that codon of the target, and events = [(kind, codon)]: q1 / q2 /
    qc / q4 one base, two bases, a codon or four bases more in the query in front of that codon, t1 / t2 / tc / t4 in the target
    (an event listed twice: twice as much).  The `keep` codons
    either side of an intron are the same on both sides, so that the split codon pays.  flank_q random bases in front of the
    query (1 or 2: the region starts off frame), flank_t in front of and behind the target (None: 5 to 40)."""
    pep = [rng.choice(AA) for _ in range(n_aa)]
    qc = [rng.choice(CODONS[a]) for a in pep]
    tc = [rng.choice(CODONS[rng.choice(AA) if rng.random() < sub else a]) for a in pep]
    for ci, _, _ in introns:
        for k in range(max(0, ci - keep), min(n_aa, ci + keep + 1)):
            tc[k] = qc[k]
    qx, tx = [""] * n_aa, [""] * n_aa
    for kind, ci in events:
        extra = {"1": 1, "2": 2, "c": 3, "4": 4}[kind[1]]
        side = qx if kind[0] == "q" else tx
        side[ci] += "".join(rng.choice(CODONS[rng.choice(AA)])) if extra == 3 else dna(rng, extra)
    cut = {ci: (ph, n) for ci, ph, n in introns}
    t = []
    for k in range(n_aa):
        t.append(tx[k])
        if k in cut:
            ph, n = cut[k]
            t.append(tc[k][:ph] + intron(rng, n) + tc[k][ph:])
        else:
            t.append(tc[k])
    q = dna(rng, flank_q) + "".join(x + c for x, c in zip(qx, qc))
    ft = (rng.randint(5, 40), rng.randint(5, 40)) if flank_t is None else (flank_t, flank_t)
    return q, dna(rng, ft[0]) + "".join(t) + dna(rng, ft[1])


def query_of_length(rng, qlen, **kw):
    """gene_pair with a query of exactly qlen bases: qlen // 3 codons behind qlen % 3 random bases."""
    q, t = gene_pair(rng, qlen // 3, flank_q=qlen % 3, **kw)
    assert len(q) == qlen
    return q, t


STRIP = 192                     # query rows of one strip (64 lanes x R = 3 rows per lane, tools/gen_kernel_tus.py)


def strip_edge_pair(rng, boundary, phase, first_row):
    """A pair whose path holds one intron of `phase` (1 or 2) whose split codon starts at query row `first_row` (near `boundary`):
    a query of boundary + 60 bases or so in frame `first_row % 3`, a target of about 700 bases with one intron of 60 to 90."""
    flank = first_row % 3
    ci = (first_row - flank) // 3
    n_aa = ci + 20
    q, t = gene_pair(rng, n_aa, introns=[(ci, phase, rng.randint(60, 90))], flank_q=flank, flank_t=0, sub=0.03, keep=4)
    pad = max(0, 700 - len(t))
    return q, dna(rng, pad // 2) + t + dna(rng, pad - pad // 2)


def split_codon_rows(model, aln):
    """[(phase, first query row of the split codon)] of alignment dict `aln`: the row at which the pre-intron transition starts."""
    m, out = model.c, []
    i = aln["region"][0]
    for tr, length in aln["ops"]:
        d = m.transitions[tr]
        name = d.name.decode()
        if name.startswith("(START) to phase"):
            out.append((int(name[len("(START) to phase")]), i))
        i += d.advance_query * length
    return out


def fuzz_pair(rng):
    """Like tests/test_gpu_codon.py's _fuzz_pair -- homologous coding sequences with substitutions, codon indels, one- and two-base
    frameshifts on either axis, flanks of 0 to 5 bases, now and then an N, an ambiguity code, a stop codon or lower case -- with
    zero to two GT ... AG introns of 30 to 120 bases put into the target at any phase."""
    n = rng.choice([1, 2, 5, 6, 7, 12, 20, 35, 60, 100, 150])
    pep = [rng.choice(AA) for _ in range(n)]
    qc = [rng.choice(CODONS[a]) for a in pep]
    tc = [rng.choice(CODONS[rng.choice(AA + "*") if rng.random() < 0.1 else a]) for a in pep]
    for _ in range(rng.choice([0, 1, 1, 2]) if n >= 12 else 0):
        at = rng.randrange(2, n - 2)
        ph = rng.randrange(3)
        for k in range(at - 2, at + 3):
            tc[k] = qc[k]
        tc[at] = tc[at][:ph] + intron(rng, rng.randint(30, 120)) + tc[at][ph:]
    for side in (qc, tc):
        for _ in range(rng.choice([0, 0, 1, 2])):
            if not side:
                break
            at = rng.randrange(len(side))
            kind = rng.randrange(4)
            if kind == 0:
                side[at:at] = [rng.choice(CODONS[rng.choice(AA)]) for _ in range(rng.randint(1, 3))]
            elif kind == 1 and len(side[at]) == 3:
                del side[at]
            elif kind == 2:
                side[at] += dna(rng, rng.randint(1, 2))
            elif len(side[at]) == 3:
                side[at] = side[at][:rng.randint(1, 2)]
    out = []
    for s in ("".join(qc), "".join(tc)):
        s = dna(rng, rng.randint(0, 5)) + s + dna(rng, rng.randint(0, 5))
        if rng.random() < 0.25:
            s = "".join(rng.choice("NRYKMSW") if rng.random() < 0.03 else c for c in s)
        if rng.random() < 0.2:
            s = s.lower() if rng.random() < 0.5 else s[:len(s) // 2] + s[len(s) // 2:].lower()
        out.append(s or "A")
    return tuple(out)


FUZZ_SEED = 20261                # checked with refdump: at least 10 of the 60 reference paths hold an intron, each phase at least twice
FUZZ_POINTS = [("default", 32), ("altparams", 0), ("cheap", 32)]
EDGE_SEED = 515                  # checked with refdump: all 32 strip-edge pairs take the intended phase's intron at the intended row
