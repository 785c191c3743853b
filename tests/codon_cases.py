"""The vector sets of the translated models -- ungapped:trans (src/model/ungapped.c:106-166 with Match_Type_CODON2CODON) and
coding2coding (src/model/coding2coding.c:50-66) -- and their loaders, shared by the codon tests (data and plumbing only; no
reference code).  Both kinds are made by tools/make_golden.py:
  * refdump-made (tests/golden/coding2coding*.jsonl, ungapped_trans*.jsonl): records of the reference's Optimal_find_score /
    Optimal_find_path, default parameters and the point CODONALT_FLAGS, -D 32 and -D 0, with the sub-optimal loop.
  * reference-binary-made (tests/golden/codon_cli_*.json): inputs and stdout of `exonerate --model <m> --exhaustive yes --subopt no
    -n 1` with every report switched on, one run per pair, two of them with their best alignment on a minus strand; beside each,
    the same alignment as transition ids (refdump on the strands the binary chose).
The CPU oracle has no 3:3 match, so the reference's records are the only yardstick here.
"""
import json, os

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


__all__ = ["REFDUMP_SETS", "SUBOPT_SETS", "CLI_SETS", "SUBOPT_MAX", "CODONALT_FLAGS", "MODEL_NAME", "set_model", "load_cli",
           "cli_lines", "recorded_alignment", "strand_seqs", "revcomp", "replay", "codon_code", "load_set", "_abi"]
