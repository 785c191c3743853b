"""The printers on paths with NER operations: the CPU oracle's alignments at the parameter points of the reference-binary-made ner
sets (tests/golden/ner_cli_*.json, tests/ner_cases.py), formatted by the library's host-only entry points, against the lines the
reference binary printed: sugar, cigar, vulgar (`N q t`, alignment.c:1725-1729), the alignment display with its
`--< NER n >--` blocks (alignment.c:774-812,1147-1159), both GFF dumps and a --ryo line.  Text: every comparison is exact."""
import ctypes as C
import difflib

import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
from ner_cases import CLI_SETS, load_cli, cli_lines, oracle_alignment, vulgar_labels, ner_block_crosses_a_line_break


def _diff(got, ref):
    return "\n".join(list(difflib.unified_diff(ref, got, "reference", "library", lineterm=""))[:60])


@pytest.mark.parametrize("name", CLI_SETS)
def test_printed_lines_are_the_reference_s(name):
    data, model = load_cli(name)
    assert len(data["pairs"]) >= 2
    for pair in data["pairs"]:
        aln = oracle_alignment(model, pair["query"], pair["target"])
        got = cli_lines(data, pair, aln)
        assert got == pair["stdout"], pair["id"] + "\n" + _diff(got, pair["stdout"])


def _recorded(name, prefix):
    data, _ = load_cli(name)
    return [[l for l in pair["stdout"] if l.startswith(prefix)][0] for pair in data["pairs"]]


def test_the_sets_hold_what_they_are_for():
    """So that the sets cannot rot: gaps and NERs in one path, a NER block across a line break of the display, every irregularity
    a NER under huge gap penalties, none under a huge ner penalty."""
    mixed = [v for name in ("ner_cli_default", "ner_cli_open35") for v in _recorded(name, "vulgar:") if {"G", "N"} <= vulgar_labels(v)]
    assert mixed
    assert any(ner_block_crosses_a_line_break(pair["stdout"]) for name in CLI_SETS for pair in load_cli(name)[0]["pairs"])
    for v in _recorded("ner_cli_hugegap", "vulgar:"):
        assert vulgar_labels(v) == {"M", "N"}, v
    for v in _recorded("ner_cli_hugeopen", "vulgar:"):
        assert "N" not in vulgar_labels(v), v
    assert any("G" in vulgar_labels(v) for v in _recorded("ner_cli_hugeopen", "vulgar:"))
    for v in _recorded("ner_cli_protein", "vulgar:"):
        assert "N" in vulgar_labels(v) and v.split()[4] == "."


def test_gff_gene_output_refuses_a_ner_path(lib):
    """Where the reference aborts on the label ("Unexpected NER for gff gene output", alignment.c:3104-3105) the library
    returns an error and says why."""
    data, model = load_cli("ner_cli_default")
    pair = data["pairs"][0]
    aln = oracle_alignment(model, pair["query"], pair["target"])
    with pytest.raises(ex.C4GpuError):
        aln.gff(pair["query"], pair["target"], genomic=True)
    assert b"Unexpected NER" in lib.c4gpu_last_error()
