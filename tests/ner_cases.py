"""The ner (non-equivalenced regions, src/model/ner.c) vector sets and their loaders, shared by the ner tests (data and plumbing
only; no reference code).

Two kinds of sets, both made by tools/make_golden.py:
  * refdump-made (tests/golden/ner_*_open0*.jsonl): records of the reference's Optimal_find_score / Optimal_find_path.  refdump
    does not register the NER argument set, so these are the parameter point --neropen 0.
  * reference-binary-made (tests/golden/ner_cli_*.json): the inputs and the stdout lines of
    `exonerate --model ner --exhaustive yes --subopt no -n 1 <flags>` with every report switched on, one run per pair, at the
    penalties refdump cannot reach (the default -20, -35, huge gaps, a huge ner penalty) and for protein.
"""
import json, os

import exonerate_amd as ex
from exonerate_amd import _abi
from golden_util import GOLDEN_DIR, apply_flags, load_set

# set -> (query alphabet, target alphabet); every one of them at ner open penalty 0
REFDUMP_SETS = {"ner_dna_open0": (0, 0), "ner_protein_open0": (1, 1), "ner_dna_open0_D0": (0, 0)}
# ... with the GAM sub-optimal loop (rec["subopt"], rec["threshold"]; --suboptmax 4: at most SUBOPT_MAX alignments per pair)
SUBOPT_SETS = {"ner_dna_open0_subopt": (0, 0), "ner_dna_open0_subopt_D0": (0, 0)}
# ... with a CDS annotation on the query (rec["cds"], exonerate's --annotation: no 1:1 DNA match inside it)
ANNOT_SETS = {"ner_dna_open0_annot": (0, 0), "ner_dna_open0_annot_D0": (0, 0)}
CLI_SETS = ["ner_cli_default", "ner_cli_open35", "ner_cli_protein", "ner_cli_hugegap", "ner_cli_hugeopen"]
NER_OPEN_DEFAULT = -20           # ner.c:31-33
SUBOPT_MAX = 4


def open0_model(name):
    qa, ta = REFDUMP_SETS[name] if name in REFDUMP_SETS else ANNOT_SETS[name] if name in ANNOT_SETS else SUBOPT_SETS[name]
    return ex.Model("ner", query_alphabet=qa, target_alphabet=ta, ner_open=0)


def load_cli(name):
    """(set, model): the recorded runs of one parameter point and the model at that point."""
    with open(os.path.join(GOLDEN_DIR, name + ".json")) as f:
        data = json.load(f)
    flags, ner_open = [], None
    for k in range(0, len(data["flags"]), 2):
        if data["flags"][k] == "--neropen":
            ner_open = int(data["flags"][k + 1])
        else:
            flags += data["flags"][k:k + 2]
    params = apply_flags(ex.default_params(), flags)
    a = 1 if data["alphabet"] == "protein" else 0
    return data, ex.Model("ner", query_alphabet=a, target_alphabet=a, params=params, ner_open=ner_open)


def cli_lines(data, pair, aln):
    """The stdout lines of the recorded run of `pair`, printed by the library's printers for alignment `aln` (an
    exonerate_amd.Alignment, whoever computed it), without the ##date line the recording dropped."""
    strand = "." if data["alphabet"] == "protein" else "+"
    q, t, qid, tid = pair["query"], pair["target"], pair["id"], pair["tid"]
    text = aln.display(q, t, qid, tid, strand, strand, qdef=pair["qdef"])
    text += aln.sugar(qid, tid, strand, strand) + "\n" + aln.cigar(qid, tid, strand, strand) + "\n"
    text += aln.vulgar(qid, tid, strand, strand) + "\n"
    text += aln.gff(q, t, qid, tid, strand, strand, on_query=True, result_id=0)
    text += aln.gff(q, t, qid, tid, strand, strand, on_query=False, result_id=0)
    text += aln.ryo(data["ryo"], q, t, qid, tid, strand, strand, qdef=pair["qdef"])
    text += "-- completed exonerate analysis\n"
    return [l for l in text.split("\n") if not l.startswith("##date ")]


def oracle_alignment(model, q, t, dpmemory=32):
    """Optimal_find_path of the CPU oracle as an exonerate_amd.Alignment (the printers need no device)."""
    import oracle_lib
    d = oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=dpmemory)
    assert d is not None
    return ex.Alignment.from_parts(model, d["score"], d["region"], d["ops"], len(q), len(t))


def vulgar_labels(line):
    f = line.split()[10:]
    return set(f[0::3])


def ner_block_crosses_a_line_break(lines):
    """Does some row of the alignment display end inside a `--< .. >--` block (AlignmentView_add_NER's string is not
    split by the view, the rows are cut at the display width)?"""
    for l in lines:
        if " : " not in l or not l.startswith(" "):
            continue
        parts = l.split(" : ")
        if len(parts) == 3 and parts[1].count("--<") != parts[1].count(">--"):
            return True
    return False


__all__ = ["REFDUMP_SETS", "SUBOPT_SETS", "ANNOT_SETS", "CLI_SETS", "NER_OPEN_DEFAULT", "SUBOPT_MAX", "open0_model", "load_cli", "cli_lines",
           "oracle_alignment", "vulgar_labels", "ner_block_crosses_a_line_break", "load_set", "_abi"]
