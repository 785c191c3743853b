"""The opt-in codon seeding of the drop-in binary (C4GPU_CODON_SEED=1: heuristic ungapped:trans and coding2coding runs through
the HSP and word-scan seams), checked WITHOUT a device: with C4GPU_HSP_HOST=1 / C4GPU_SEED_HOST=1 the extensions are the
reference's own HSPset_seed_hsp on scratch sets and the scan a dictionary walk, so the seams' own work -- taking codon sets and
translated seeders, the chains, the replay on the set's horizon, the fused route's delivery -- is exercised byte for byte against
the unmodified reference.  Without the switch nothing moves.  The device route: test_gpu_codon_seed_dropin.py."""
import json
import os
import re
import subprocess

import pytest

from golden_util import GOLDEN_DIR
from test_gpu_codon_dropin import _inputs, _write, GPU_EXE, CPU_EXE
from test_softmask_dropin_host import hsp_line
from test_integration_seed_fused_host import fused_line

pytestmark = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                reason="reference binaries are built in the build container (make -C integration)")

HOST = {"C4GPU_HSP_HOST": "1", "C4GPU_SEED_HOST": "1", "C4GPU_SDP_HOST": "1", "C4GPU_BSDP_HOST": "1", "C4GPU_SEED_FACTOR": "0"}
SWITCH = dict(HOST, C4GPU_CODON_SEED="1")
SHOW = ["--showalignment", "yes", "--showvulgar", "yes", "--showsugar", "yes", "-V", "0"]
# the five runs: (model and options, soft-masked input, seams in use)
RUNS = {
    "trans": (["-m", "ungapped:trans", "--score", "30"], False, "both"),
    "trans_softmasktarget": (["-m", "ungapped:trans", "--score", "30", "--softmasktarget", "yes"], True, "both"),
    "trans_softmaskboth": (["-m", "ungapped:trans", "--score", "30", "--softmaskquery", "yes", "--softmasktarget", "yes"], True, "hsp"),
    "coding2coding_sdp": (["-m", "coding2coding"], False, "both"),
    "coding2coding_bsdp": (["-m", "coding2coding", "--gappedextension", "no"], False, "both"),
}


def codon_inputs(masked):
    """Homologous coding pairs (the inputs of test_gpu_codon_dropin.py) and the inputs the fixtures were recorded from: wrapped
    seeds, shared entries, HSPs at the very ends.  masked: the lower-case target of the fixtures and lower-case runs in others."""
    with open(os.path.join(GOLDEN_DIR, "codon_hsp_cli.json")) as f:
        cli = json.load(f)["runs"]
    qs, ts = _inputs(5, 3, lo=60, hi=90)
    for name in ("A", "D", "E"):
        qs.append(("q" + name, cli[name]["query"]))
    for name in ("A", "C", "D", "E"):
        ts.append(("t" + name, cli[name]["target"]))
    if masked:
        low = lambda s: "".join(c.lower() if (i // 21) % 3 == 1 else c for i, c in enumerate(s))
        ts = [(n, low(t)) for n, t in ts] + [("tB", cli["B_t"]["target"])]
    return qs, ts


def run(tmp_path, name, env, extra=()):
    args, masked, _ = RUNS[name]
    qf, tf = _write(tmp_path, *codon_inputs(masked))
    args = args + SHOW + list(extra) + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **env))
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return ref.stdout, gpu.stdout, gpu.stderr.decode()


def seed_line(err):
    m = re.search(r"c4gpu seed: (\d+) targets walked in (\d+) device scans \((\d+) symbols\): (\d+) word hits", err)
    assert m, err[-1500:]
    return [int(x) for x in m.groups()]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_runs_are_byte_identical_and_served_by_both_seams(tmp_path, name):
    seams = RUNS[name][2]
    env = dict(SWITCH, C4GPU_SEED_CHECK="1") if seams == "both" else dict(SWITCH, C4GPU_SEED_OFF="1")
    ref, gpu, err = run(tmp_path, name, env)
    assert gpu == ref and ref.count(b"vulgar:") >= 6
    line = hsp_line(err)
    assert line["hits"] > 200 and line["stored"] > 0 and line["sets"] >= 6
    if RUNS[name][1]:
        assert line["dropped"] >= 6, err[-600:]
    if seams == "both":
        targets, _, _, hits = seed_line(err)
        assert targets > 0 and hits == line["hits"]
        assert "every seed equal to the reference's own walk" in err
    else:
        assert "targets walked in" not in err


@pytest.mark.parametrize("name", ["trans", "coding2coding_sdp", "coding2coding_bsdp"])
def test_fused_route_is_byte_identical_with_host_sets(tmp_path, name):
    ref, gpu, err = run(tmp_path, name, dict(SWITCH, C4GPU_SEED_FUSED="1"))
    assert gpu == ref and ref.count(b"vulgar:") >= 6
    targets, hits, extended, kept = fused_line(err)
    assert targets > 0 and hits > 200 and hits > extended >= kept > 0
    assert "c4gpu hsp:" not in err and "takes the scan and extension calls" not in err


@pytest.mark.parametrize("name", ["trans", "coding2coding_sdp"])
def test_without_the_switch_nothing_moves(tmp_path, name):
    """The default: no seam serves a heuristic translated run, in host mode either, fused or not."""
    ref, gpu, err = run(tmp_path, name, dict(HOST, C4GPU_SEED_FUSED="1"))
    assert gpu == ref
    assert "c4gpu hsp:" not in err and "targets walked in" not in err and fused_line(err)[0] == 0


def test_a_run_with_an_annotation_file_is_the_references(tmp_path):
    """--annotation: Match_3_3_split_score_func vetoes codons outside the CDS frame inside the score, which the coded arrays
    do not know -- a set whose query carries an annotation (and, fused, a seeder with such a query) stays with the reference.
    A run with an annotation file is the reference's, byte for byte, on both routes."""
    qs, _ = codon_inputs(False)
    ann = str(tmp_path / "cds.txt")
    with open(ann, "w") as f:
        f.write("%s + 4 60\n" % qs[0][0])
    for env in (SWITCH, dict(SWITCH, C4GPU_SEED_FUSED="1")):
        ref, gpu, err = run(tmp_path, "trans", env, extra=["--annotation", ann])
        assert gpu == ref and ref.count(b"vulgar:") >= 4
