"""The translated models -- ungapped:trans and coding2coding, match advance 3/3 -- on the MI355X: the FAM_UNGAPPED_CODON and
FAM_CODING2CODING instantiations of the Viterbi kernels (kernels/k_ungapped_codon_*.hip, k_coding2coding_*.hip: lanes hand their
last three query rows down, c4_viterbi_kernel.h WaveDP::AQ) through the engine's public calls, against records of the reference
itself (tests/golden/coding2coding*.jsonl, ungapped_trans*.jsonl), against the lines the reference binary printed
(tests/golden/codon_cli_*.json) and, for fresh random pairs, against the reference's refdump run on the spot (oracle/_ref/refdump,
built by build()).  Integer work and text: every comparison is exact."""
import json
import os
import random
import re
import subprocess
import tempfile

import pytest

import exonerate_amd as ex
from golden_util import expected, apply_flags
from codon_cases import (REFDUMP_SETS, SUBOPT_SETS, CLI_SETS, SUBOPT_MAX, CODONALT_FLAGS, set_model, load_set, load_cli,
                         cli_lines, strand_seqs)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
FAMILY_TAG = {"coding2coding": "_coding2coding_", "ungapped:trans": "_ungapped_codon_"}


def _kernels(err):
    """names of the kernels a traced call launched (C4GPU_TRACE: `c4gpu trace:   kernel <name>: <n> workgroups per CU`)"""
    return re.findall(r"c4gpu trace:   kernel (k\w+):", err)


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(REFDUMP_SETS))
def test_find_score_and_path_match_reference_vectors(eng, name, monkeypatch, capfd):
    """Score, region and operation list of every record: default memory and -D 0 (checkpoints and continuations), queries of 1 to
    5, 18 and 19 bases, queries of two and three 256-row strips, batches that mix all of these lengths."""
    model = set_model(name)
    recs = load_set(name)
    pairs = [(r["query"], r["target"]) for r in recs]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    assert eng.find_score(model, pairs) == [r["score"] for r in recs]
    launched = _kernels(capfd.readouterr().err)
    assert launched and all(FAMILY_TAG[REFDUMP_SETS[name]] in k for k in launched), launched     # find_score alone: the score pass
    assert all("_score" in k for k in launched), launched
    alns = eng.find_path(model, pairs, dpmemory=recs[0]["dpmemory"])
    launched = _kernels(capfd.readouterr().err)
    assert launched and all(FAMILY_TAG[REFDUMP_SETS[name]] in k for k in launched), launched
    if name.endswith("_D0"):
        assert any("_ckpt_cont" in k for k in launched) and any("_path_cont" in k for k in launched), launched
    for rec, aln in zip(recs, alns):
        assert aln is not None and aln.as_dict(rec["id"]) == expected(rec), rec["id"]


@pytest.mark.parametrize("name", ["coding2coding", "coding2coding_D0", "ungapped_trans_D0"])
def test_resident_batch_matches_reference_vectors(eng, name):
    model = set_model(name)
    recs = load_set(name)
    b = ex.ResidentBatch(eng, model, [(r["query"], r["target"]) for r in recs])
    b.run(0)
    assert b.scores()[0] == [r["score"] for r in recs]
    b.run(2, dpmemory=recs[0]["dpmemory"])
    for i, rec in enumerate(recs):
        assert b.alignment(i).as_dict(rec["id"]) == expected(rec), rec["id"]
    b.close()


@pytest.mark.parametrize("name", sorted(SUBOPT_SETS))
def test_suboptimal_loop_matches_reference_vectors(eng, name):
    """GAM_Result_exhaustive_create's loop with SubOpt blocking (the `_sub` kernels; a 3/3 match blocks the three cells of its
    diagonal): the successive alignments the reference produced."""
    model = set_model(name)
    recs = load_set(name)
    pairs = [(r["query"], r["target"]) for r in recs]
    dpm, thr = recs[0]["dpmemory"], recs[0]["threshold"]
    found = eng.find_all_paths(model, pairs, dpmemory=dpm, threshold=thr, max_paths=SUBOPT_MAX)
    for rec, alns in zip(recs, found):
        assert [(a.score, list(a.region), [list(o) for o in a.ops], a.vulgar(rec["id"])) for a in alns] == \
               [(e["path_score"], e["region"], e["ops"], e["vulgar"]) for e in rec["subopt"]], rec["id"]


def test_local_shortcut_off_gives_the_same_batch(eng, monkeypatch, capfd):
    """C4GPU_LOCAL_EXACT=0 and C4GPU_CONT_FREE=0 (the existing test hooks) send every pass to the kernels that keep the validity
    masks -- for an advance of a: i - a >= 0 -- and C4GPU_PACK=0 to the two-slot region start: same alignments either way."""
    model = ex.Model("coding2coding")
    recs = load_set("coding2coding_D0")
    pairs = [(r["query"], r["target"]) for r in recs]
    monkeypatch.setenv("C4GPU_TRACE", "1")

    def run():
        out = [a.as_dict(r["id"]) for a, r in zip(eng.find_path(model, pairs, dpmemory=0), recs)]
        return out, _kernels(capfd.readouterr().err)
    on = run()
    monkeypatch.setenv("C4GPU_LOCAL_EXACT", "0")
    monkeypatch.setenv("C4GPU_CONT_FREE", "0")
    monkeypatch.setenv("C4GPU_PACK", "0")
    off = run()
    assert any("_local" in k for k in on[1]) and not any("_local" in k or "_pack" in k for k in off[1]), (on[1], off[1])
    assert on[0] == off[0] == [expected(r) for r in recs]


@pytest.mark.parametrize("name", CLI_SETS)
def test_cli_sets_print_as_the_reference_binary_did(eng, name):
    """Both strands: the device aligns the sequences as the recorded run read them, and the printers give the recorded stdout."""
    data, model = load_cli(name)
    pairs = [strand_seqs(p) for p in data["pairs"]]
    alns = eng.find_path(model, pairs, dpmemory=32)
    for pair, a in zip(data["pairs"], alns):
        assert (a.score, list(a.region), [list(o) for o in a.ops]) == (pair["score"], pair["region"], pair["ops"]), pair["id"]
        assert cli_lines(data, pair, a) == pair["stdout"], pair["id"]


def test_set_annotation_is_refused_on_a_codon_batch(eng, lib):
    """The 3:3 match's annotation veto depends on the frame (match.c:513-519) and is not built: an error, not a wrong score."""
    for kind in ("coding2coding", "ungapped:trans"):
        b = ex.ResidentBatch(eng, ex.Model(kind), [("ATGGCTGCTAAAGGT", "ATGGCTGCTAAAGGT")])
        with pytest.raises(ex.C4GpuError):
            b.set_annotation([(3, 9)])
        assert b"annotation" in lib.c4gpu_last_error() and b"codon" in lib.c4gpu_last_error()
        b.run(0)
        assert b.scores()[0][0] > 0
        b.close()


# ---- live fuzz against the reference ----------------------------------------------------------------------------------
AA = "ARNDCQEGHILKMFPSTWYV"
_NCBI = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODONS = {}
for _i, _a in enumerate("TCAG"):
    for _j, _b in enumerate("TCAG"):
        for _k, _c in enumerate("TCAG"):
            CODONS.setdefault(_NCBI[_i * 16 + _j * 4 + _k], []).append(_a + _b + _c)


def _fuzz_pair(rng):
    """Homologous coding sequences: substitutions, codon indels, one- and two-base frameshifts on either axis, flanks of 0 to 5
    bases, now and then an N, an ambiguity code, a stop codon or lower case."""
    n = rng.choice([1, 2, 5, 6, 7, 12, 20, 35, 60, 100, 150])
    pep = [rng.choice(AA) for _ in range(n)]
    qc = [rng.choice(CODONS[a]) for a in pep]
    tc = [rng.choice(CODONS[rng.choice(AA + "*") if rng.random() < 0.1 else a]) for a in pep]
    for side in (qc, tc):
        for _ in range(rng.choice([0, 0, 1, 2])):
            if not side:
                break
            at = rng.randrange(len(side))
            kind = rng.randrange(4)
            if kind == 0:
                side[at:at] = [rng.choice(CODONS[rng.choice(AA)]) for _ in range(rng.randint(1, 3))]
            elif kind == 1:
                del side[at]
            elif kind == 2:
                side[at] += "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 2)))
            elif len(side[at]) == 3:
                side[at] = side[at][:rng.randint(1, 2)]
    out = []
    for s in ("".join(qc), "".join(tc)):
        s = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 5))) + s + "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 5)))
        if rng.random() < 0.25:
            s = "".join(rng.choice("NRYKMSW") if rng.random() < 0.03 else c for c in s)
        if rng.random() < 0.2:
            s = s.lower() if rng.random() < 0.5 else s[:len(s) // 2] + s[len(s) // 2:].lower()
        out.append(s or "A")
    return tuple(out)


def _refdump(model_type, cases, dpmemory, flags):
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as f:
        for c in cases:
            f.write("%s\t%s\t%s\n" % c)
        path = f.name
    try:
        out = subprocess.run([REFDUMP, "--cmd", "golden", "--model", model_type, "--input", path, "-D", str(dpmemory)] + list(flags),
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, timeout=300).stdout.decode()
    finally:
        os.unlink(path)
    recs = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert [r["id"] for r in recs] == [c[0] for c in cases]
    return recs


@pytest.mark.skipif(not os.path.exists(REFDUMP), reason="oracle/_ref/refdump is built by build() where the reference tree is")
@pytest.mark.parametrize("model_type", ["coding2coding", "ungapped:trans"])
def test_live_fuzz_against_the_reference(eng, model_type):
    """60 fixed-seed random pairs per model in three parameter sets (default, CODONALT_FLAGS, a cheap frameshift), -D 32 and
    -D 0: scores, regions and operation lists equal to what the reference computes for the same input, all of them compared."""
    rng = random.Random(20250 + len(model_type))
    points = [([], 32), (CODONALT_FLAGS, 0), (["--frameshift", "-9", "--codongapopen", "-20", "--codongapextend", "-2"], 32)]
    compared = 0
    for flags, dpm in points:
        cases = [("fz%03d" % k, ) + _fuzz_pair(rng) for k in range(20)]
        recs = _refdump(model_type, cases, dpm, flags)
        model = ex.Model(model_type, params=apply_flags(ex.default_params(), flags))
        pairs = [(c[1], c[2]) for c in cases]
        assert eng.find_score(model, pairs) == [r["score"] for r in recs], flags
        for c, rec, aln in zip(cases, recs, eng.find_path(model, pairs, dpmemory=dpm)):
            assert rec["ops"] and aln is not None, c
            assert aln.as_dict(rec["id"]) == expected(rec), (flags, c)
            compared += 1
    assert compared == 60
