"""The printers on paths of the translated models (match advance 3/3, Match_3_3_display_func): the reference's own alignments as
transition ids, formatted by the library's host-only entry points, against what the reference printed -- sugar, cigar and vulgar of
every refdump-made record (codon `C q t`, frameshift `F q t`, codon gaps `G 3n 0`), and for the reference-binary-made sets
(tests/golden/codon_cli_*.json) the whole stdout: the alignment display with both sequences translated, both GFF dumps and a --ryo
line, on plus and minus strands.  Text: every comparison is exact."""
import difflib

import pytest

import exonerate_amd as ex
from codon_cases import REFDUMP_SETS, SUBOPT_SETS, CLI_SETS, set_model, load_set, load_cli, cli_lines, recorded_alignment


def _diff(got, ref):
    return "\n".join(list(difflib.unified_diff(ref, got, "reference", "library", lineterm=""))[:60])


@pytest.mark.parametrize("name", sorted(REFDUMP_SETS))
def test_sugar_cigar_vulgar_of_the_recorded_paths(name):
    model = set_model(name)
    for rec in load_set(name):
        aln = ex.Alignment.from_parts(model, rec["path_score"], rec["region"], rec["ops"], rec["qlen"], rec["tlen"])
        assert (aln.sugar(rec["id"]), aln.cigar(rec["id"]), aln.vulgar(rec["id"])) == (rec["sugar"], rec["cigar"], rec["vulgar"]), rec["id"]


@pytest.mark.parametrize("name", sorted(SUBOPT_SETS))
def test_vulgar_of_the_suboptimal_paths(name):
    model = set_model(name)
    for rec in load_set(name):
        for a in rec["subopt"]:
            aln = ex.Alignment.from_parts(model, a["path_score"], a["region"], a["ops"], rec["qlen"], rec["tlen"])
            assert aln.vulgar(rec["id"]) == a["vulgar"], rec["id"]


@pytest.mark.parametrize("name", CLI_SETS)
def test_printed_lines_are_the_reference_s(name):
    data, model = load_cli(name)
    assert len(data["pairs"]) >= 4
    for pair in data["pairs"]:
        got = cli_lines(data, pair, recorded_alignment(model, pair))
        assert got == pair["stdout"], pair["id"] + "\n" + _diff(got, pair["stdout"])


def test_the_sets_hold_what_they_are_for():
    """So that the sets cannot rot: frameshifts and codon gaps in printed paths, both minus strands, a display with translations."""
    labels, strands = set(), set()
    for name in CLI_SETS:
        for pair in load_cli(name)[0]["pairs"]:
            v = [l for l in pair["stdout"] if l.startswith("vulgar:")][0].split()
            labels |= set(v[10::3])
            strands.add((v[4], v[8]))
            assert any("Model: " in l for l in pair["stdout"]) and any(l.startswith("ryo: ") for l in pair["stdout"])
    assert {"C", "G", "F"} <= labels and {("+", "+"), ("+", "-"), ("-", "+")} <= strands
