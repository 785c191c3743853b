"""coding2genome -- coding2coding with target introns in three phases and split codons either side -- on the MI355X: the
FAM_CODING2GENOME instantiations of the Viterbi kernels (kernels/k_coding2genome_*.hip: one wave per job, three rows per lane, the
codon match's three-row hand-down together with the intron shadow and its base slot) through the engine's public calls, against
records of the reference itself (tests/golden/coding2genome*.jsonl), against the lines the reference binary printed
(tests/golden/codon_cli_coding2genome.json) and, for pairs made here, against the reference's refdump run on the spot
(oracle/_ref/refdump, built by build()).  No CPU oracle stands between: its split-codon calc is the protein query's.  Integer work
and text: every comparison is exact."""
import json
import os
import random
import re
import subprocess
import tempfile

import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
from golden_util import expected, load_set
from coding2genome_cases import (SETS, SUBOPT_SET, SUBOPT_MAX, POINT_FLAGS, FUZZ_SEED, FUZZ_POINTS, EDGE_SEED, STRIP, point_model,
                                 load_cli, revcomp, introns_of, gene_pair, strip_edge_pair, split_codon_rows, fuzz_pair, CODONS, dna,
                                 intron)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
needs_refdump = pytest.mark.skipif(not os.path.exists(REFDUMP), reason="oracle/_ref/refdump is built by build() where the reference tree is")


def _kernels(err):
    return re.findall(r"c4gpu trace:   kernel (k\w+):", err)


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


def _by_point(recs):
    out = {}
    for r in recs:
        out.setdefault(r.get("point", "default"), []).append(r)
    return sorted(out.items())


@pytest.mark.parametrize("name", sorted(SETS))
def test_find_score_and_path_match_reference_vectors(eng, name, monkeypatch, capfd):
    """Score, region, operation list and sugar / cigar / vulgar of every record, at the set's dpmemory; only kernels of the family."""
    monkeypatch.setenv("C4GPU_TRACE", "1")
    for point, recs in _by_point(load_set(name)):
        model = point_model(point)
        pairs = [(r["query"], r["target"]) for r in recs]
        assert eng.find_score(model, pairs) == [r["score"] for r in recs], point
        launched = _kernels(capfd.readouterr().err)
        assert launched and all("_coding2genome_score" in k for k in launched), launched
        alns = eng.find_path(model, pairs, dpmemory=SETS[name])
        launched = _kernels(capfd.readouterr().err)
        assert launched and all("_coding2genome_" in k for k in launched), launched
        if name.endswith("_D0"):
            assert any("_ckpt_cont" in k for k in launched) and any("_path_cont" in k for k in launched), launched
        for rec, aln in zip(recs, alns):
            assert aln is not None and aln.as_dict(rec["id"]) == expected(rec), (point, rec["id"])


@pytest.mark.parametrize("name", sorted(SETS))
def test_resident_batch_matches_reference_vectors(eng, name):
    for point, recs in _by_point(load_set(name)):
        b = ex.ResidentBatch(eng, point_model(point), [(r["query"], r["target"]) for r in recs])
        b.run(0)
        assert b.scores()[0] == [r["score"] for r in recs]
        b.run(2, dpmemory=SETS[name])
        for i, rec in enumerate(recs):
            assert b.alignment(i).as_dict(rec["id"]) == expected(rec), (point, rec["id"])
        b.close()


def test_suboptimal_loop_matches_reference_vectors(eng):
    model = point_model("default")
    recs = load_set(SUBOPT_SET)
    pairs = [(r["query"], r["target"]) for r in recs]
    found = eng.find_all_paths(model, pairs, dpmemory=recs[0]["dpmemory"], threshold=recs[0]["threshold"], max_paths=SUBOPT_MAX)
    for rec, alns in zip(recs, found):
        assert [(a.score, list(a.region), [list(o) for o in a.ops], a.vulgar(rec["id"])) for a in alns] == \
               [(e["path_score"], e["region"], e["ops"], e["vulgar"]) for e in rec["subopt"]], rec["id"]


def test_local_shortcut_off_gives_the_same_batch(eng, monkeypatch, capfd):
    """C4GPU_LOCAL_EXACT=0, C4GPU_CONT_FREE=0 and C4GPU_PACK=0: the general forms, which keep every validity mask, and the two-slot
    region start give the same alignments."""
    model = point_model("default")
    recs = load_set("coding2genome_D0")
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
    assert all("_coding2genome_" in k for k in on[1] + off[1])
    assert on[0] == off[0] == [expected(r) for r in recs]


def cli_lines(pair, alns, reports):
    """The stdout of the recorded run of `pair` as the library's printers give it for `alns` (in the recorded order)."""
    text = ""
    for k, (a, rec) in enumerate(zip(alns, pair["alignments"])):
        qs, ts = rec["qstrand"], rec["tstrand"]
        q = revcomp(pair["query"]) if qs == "-" else pair["query"]
        t = revcomp(pair["target"]) if ts == "-" else pair["target"]
        qdef = pair["qdef"] + (":[revcomp]" if qs == "-" else "")
        tdef = "[revcomp]" if ts == "-" else None
        text += a.display(q, t, pair["id"], pair["tid"], qs, ts, qdef=qdef, tdef=tdef)
        text += a.vulgar(pair["id"], pair["tid"], qs, ts) + "\n"
        text += a.gff(q, t, pair["id"], pair["tid"], qs, ts, on_query=False, result_id=k + 1)
    text += "-- completed exonerate analysis\n"
    return [l for l in text.split("\n") if not l.startswith("##date ")]


def test_cli_set_prints_as_the_reference_binary_did(eng):
    """Both strands: the device aligns the sequences as the recorded run read them, and the printers give the recorded stdout."""
    data = load_cli()
    model = point_model("default")
    assert {a["tstrand"] for p in data["pairs"] for a in p["alignments"]} == {"+", "-"}
    for pair in data["pairs"]:
        assert len(pair["alignments"]) == sum(l.startswith("vulgar:") for l in pair["stdout"]) >= 1
        alns = []
        for rec in pair["alignments"]:                    # the strand combinations the recorded run reported, in its order
            q = revcomp(pair["query"]) if rec["qstrand"] == "-" else pair["query"]
            t = revcomp(pair["target"]) if rec["tstrand"] == "-" else pair["target"]
            a = eng.find_path(model, [(q, t)], dpmemory=32)[0]
            assert (a.score, list(a.region), [list(o) for o in a.ops]) == (rec["score"], rec["region"], rec["ops"]), pair["id"]
            alns.append(a)
        assert cli_lines(pair, alns, data["reports"]) == pair["stdout"], pair["id"]


def test_set_annotation_is_refused(eng, lib):
    b = ex.ResidentBatch(eng, point_model("default"), [("ATGGCTGCTAAAGGT", "ATGGCTGCTAAAGGT")])
    with pytest.raises(ex.C4GpuError):
        b.set_annotation([(3, 9)])
    assert b"annotation" in lib.c4gpu_last_error() and b"codon" in lib.c4gpu_last_error()
    b.run(0)
    assert b.scores()[0][0] > 0
    b.close()


# ---- pairs made here, against the reference run on the spot -----------------------------------------------------------
def _refdump_one(cases, dpmemory, flags):
    f = tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False)
    for c in cases:
        f.write("%s\t%s\t%s\n" % c)
    f.close()
    return f.name, subprocess.Popen([REFDUMP, "--cmd", "golden", "--model", "coding2genome", "--input", f.name, "-D", str(dpmemory)] + list(flags),
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _refdump(cases, dpmemory, flags=()):
    """The reference's records of `cases`, in order; the interpreted Viterbi is slow, so eight pairs per process, side by side."""
    runs = [_refdump_one(cases[k:k + 8], dpmemory, flags) for k in range(0, len(cases), 8)]
    recs = []
    for path, proc in runs:
        try:
            out, err = proc.communicate(timeout=300)
        finally:
            os.unlink(path)
        assert proc.returncode == 0, err.decode()[-1000:]
        recs += [json.loads(l) for l in out.decode().splitlines() if l.startswith("{")]
    assert [r["id"] for r in recs] == [c[0] for c in cases]
    return recs


def _compare(eng, model, cases, recs, dpm):
    pairs = [(c[1], c[2]) for c in cases]
    assert eng.find_score(model, pairs) == [r["score"] for r in recs]
    n = 0
    for c, rec, aln in zip(cases, recs, eng.find_path(model, pairs, dpmemory=dpm)):
        assert rec["ops"] and aln is not None, c
        assert aln.as_dict(rec["id"]) == expected(rec), c
        n += 1
    return n


def strip_edge_cases():
    """32 pairs: strip boundaries 192 and 384, phases 1 and 2, the split codon's first query row at boundary - 4 ... + 3."""
    rng = random.Random(EDGE_SEED)
    return [("e%d_%d_%+d" % (b, ph, off), b, ph, b + off) + strip_edge_pair(rng, b, ph, b + off)
            for b in (STRIP, 2 * STRIP) for ph in (1, 2) for off in range(-4, 4)]


@needs_refdump
@pytest.mark.parametrize("dpm", [32, 0])
def test_split_codons_at_the_strip_edges(eng, dpm):
    model = point_model("default")
    edge = strip_edge_cases()
    cases = [(cid, q, t) for cid, _, _, _, q, t in edge]
    recs = _refdump(cases, dpm)
    for (cid, b, ph, row, _, t), rec in zip(edge, recs):
        # the reference's own path takes the intended phase's intron, its split codon starting at the intended row
        assert split_codon_rows(model, rec) == [(ph, row)], (cid, split_codon_rows(model, rec))
        ins = introns_of(model, rec["ops"], rec["region"])
        assert [p for p, _, _ in ins] == [ph] and 60 <= ins[0][2] <= 90, cid
        assert 650 <= len(t) <= 800, cid
    assert _compare(eng, model, cases, recs, dpm) == 32


def _checkpoint_pair(ci, n):
    q, t = gene_pair(random.Random("ckpt/%d/%d" % (ci, n)), 64, introns=[(ci, 1 + (ci + n) % 2, n)], flank_t=7, sub=0.0)
    return ("k%d_%d" % (ci, n), q, t)


def checkpoint_features(lib, model, rec):
    """{(what, offset)}: which of the 5' site's column, the 3' site's and the column the post-intron split codon ends in lie one
    before (-1), on (0) or one behind (+1) a checkpoint column of the -D 0 pass over the record's region; the columns are those of
    the library's memory rule (c4gpu_checkpoint_rows: `rows` checkpoints, target_length // (rows + 1) columns apart)."""
    ins = introns_of(model, rec["ops"], rec["region"])
    if len(ins) != 1 or not split_codon_rows(model, rec):
        return set()
    ph, start, n = ins[0]
    region = _abi.Region(*rec["region"])
    rows = lib.c4gpu_checkpoint_rows(model.c, region, 0)
    assert lib.c4gpu_use_reduced_space(model.c, region, 0) and rows >= 1
    section = rec["region"][3] // (rows + 1)
    cols = [k * section for k in range(1, rows + 1)]                                # DP columns of the region
    j5 = start - rec["region"][1]
    feature = {"5ss": j5, "3ss": j5 + n - 2, "split": j5 + n + (2 if ph == 1 else 1)}
    return {(what, off) for what, j in feature.items() for off in (-1, 0, 1) if j - off in cols}


# (what, offset) -> (codon the intron sits in, intron length) of _checkpoint_pair: found by trying codons 24 ... 39 and lengths
# 40 ... 63 against the reference; the test asserts that each still lies where it says
CHECKPOINT_CASES = {("3ss", -1): (24, 45), ("3ss", 0): (24, 47), ("3ss", 1): (24, 49), ("5ss", -1): (38, 40), ("5ss", 0): (38, 41),
                    ("5ss", 1): (39, 43), ("split", -1): (24, 40), ("split", 0): (24, 41), ("split", 1): (24, 43)}


@needs_refdump
def test_sites_and_split_codons_at_the_checkpoint_columns(eng, lib):
    model = point_model("default")
    keys = sorted(CHECKPOINT_CASES)
    assert keys == sorted((w, o) for w in ("5ss", "3ss", "split") for o in (-1, 0, 1))
    cases = [_checkpoint_pair(*CHECKPOINT_CASES[k]) for k in keys]
    recs = _refdump(cases, 0)
    for k, rec in zip(keys, recs):
        assert k in checkpoint_features(lib, model, rec), (k, rec["id"])
    assert _compare(eng, model, cases, recs, 0) == 9


def first_row_cases():
    """Queries that begin with the last two bases or the last base of a codon whose whole codon the target carries around an
    intron: the best alignment would need a split codon that ends in query row 2 or 1, where there is none (phase.c:174-186)."""
    rng = random.Random(31)
    out = []
    for ph in (1, 2):
        for k in range(3):
            pep = [rng.choice("WCFYHM") for _ in range(14)]
            cod = [rng.choice(CODONS[a]) for a in pep]
            body = "".join(cod[1:])
            q = cod[0][ph:] + body
            t = dna(rng, 9 + k) + cod[0][:ph] + intron(rng, 40 + 5 * k) + cod[0][ph:] + body + dna(rng, 5)
            out.append(("f%d_%d" % (ph, k), q, t))
    return out


@needs_refdump
def test_no_split_codon_ends_in_the_first_rows(eng):
    model = point_model("cheap")
    cases = first_row_cases()
    for dpm in (32, 0):
        recs = _refdump(cases, dpm, POINT_FLAGS["cheap"])
        for rec in recs:                          # the reference's path: whatever it does instead, no split codon ends in rows 1 or 2
            i = rec["region"][0]
            for tr, length in rec["ops"]:
                d = model.c.transitions[tr]
                i += d.advance_query * length
                assert not (d.name.decode().startswith("phase") and i < 3), rec["id"]
            assert rec["region"][0] <= 2, rec["id"]
        assert _compare(eng, model, cases, recs, dpm) == len(cases)


@needs_refdump
def test_live_fuzz_against_the_reference(eng):
    """60 fixed-seed pairs in three parameter points: scores, regions and operation lists equal to the reference's, all compared."""
    rng = random.Random(FUZZ_SEED)
    compared, with_intron, phases = 0, 0, []
    for point, dpm in FUZZ_POINTS:
        cases = [("fz%03d" % k, ) + fuzz_pair(rng) for k in range(20)]
        recs = _refdump(cases, dpm, POINT_FLAGS[point])
        model = point_model(point)
        for rec in recs:
            ins = introns_of(model, rec["ops"], rec["region"])
            with_intron += bool(ins)
            phases += [p for p, _, _ in ins]
        compared += _compare(eng, model, cases, recs, dpm)
    assert compared == 60
    assert with_intron >= 10 and all(phases.count(p) >= 2 for p in (0, 1, 2)), (with_intron, phases)
