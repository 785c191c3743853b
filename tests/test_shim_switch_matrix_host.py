"""Which opt-in switch of the drop-in binary opens which heuristic seam, pinned as a table and checked WITHOUT a device.

Every seam runs in host mode (the batch behind it is the reference's own code), so a run shows the seams' own decisions only:
which of them collect a model's pairs under which switch.  For coding2genome and coding2coding, with and without
--gappedextension, exonerate-gpu runs with no opt-in switch and with exactly one of the five set to 1; its stdout is the
reference's byte for byte, and the seams that report on stderr (C4GPU_VERBOSE=1) are those of EXPECTED.  Two more cases give a
switch the value 2, one per truth rule: C4GPU_CODING2GENOME_BSDP means "== 1" and does not serve coding2genome at 2 (EXPECTED's
second column), C4GPU_CODING2GENOME_SDP means "nonzero" and does.

EXPECTED was recorded from the shim as it stood BEFORE its switches moved into integration/c4gpu_switches.h (the commit before
that header exists), by running this file's own commands against that binary.  It is data: when a seam's rule is changed on
purpose, change the entry by hand and say why; never regenerate it from the code under test."""
import functools
import os
import re
import subprocess

import pytest

from test_coding2genome_sdp_dropin_host import inputs
from test_codon_sdp_dropin_host import sdp_line
from test_gpu_codon_dropin import _write, GPU_EXE, CPU_EXE, REPORTS

pytestmark = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                reason="reference binaries are built in the build container (make -C integration)")

HOST = {"C4GPU_SDP_HOST": "1", "C4GPU_BSDP_HOST": "1", "C4GPU_HSP_HOST": "1", "C4GPU_SEED_HOST": "1"}
SWITCHES = ["C4GPU_CODING2GENOME", "C4GPU_CODING2GENOME_SDP", "C4GPU_CODING2GENOME_BSDP", "C4GPU_CODON_SDP", "C4GPU_CODON_SEED"]
SEAMS = ("sdp", "bsdp", "hsp", "seed")                   # recognised by "c4gpu <seam>:" on stderr
CASES = ["none"] + [s + "=1" for s in SWITCHES] + ["C4GPU_CODING2GENOME_BSDP=2", "C4GPU_CODING2GENOME_SDP=2"]

# (model, --gappedextension, case) -> (the seams that report, whether the BSDP seam served pairs: it also reports, under its
# prefix, the wide model it leaves to the reference)
EXPECTED = {
    ("coding2genome", "yes", "none"): ((), False),
    ("coding2genome", "yes", "C4GPU_CODING2GENOME=1"): ((), False),
    ("coding2genome", "yes", "C4GPU_CODING2GENOME_SDP=1"): (("sdp",), False),
    ("coding2genome", "yes", "C4GPU_CODING2GENOME_BSDP=1"): ((), False),
    ("coding2genome", "yes", "C4GPU_CODON_SDP=1"): ((), False),
    ("coding2genome", "yes", "C4GPU_CODON_SEED=1"): (("hsp", "seed"), False),
    ("coding2genome", "yes", "C4GPU_CODING2GENOME_BSDP=2"): ((), False),
    ("coding2genome", "yes", "C4GPU_CODING2GENOME_SDP=2"): (("sdp",), False),
    ("coding2genome", "no", "none"): (("bsdp",), False),
    ("coding2genome", "no", "C4GPU_CODING2GENOME=1"): (("bsdp",), False),
    ("coding2genome", "no", "C4GPU_CODING2GENOME_SDP=1"): (("bsdp",), False),
    ("coding2genome", "no", "C4GPU_CODING2GENOME_BSDP=1"): (("bsdp",), True),
    ("coding2genome", "no", "C4GPU_CODON_SDP=1"): (("bsdp",), False),
    ("coding2genome", "no", "C4GPU_CODON_SEED=1"): (("bsdp", "hsp", "seed"), False),
    ("coding2genome", "no", "C4GPU_CODING2GENOME_BSDP=2"): (("bsdp",), False),
    ("coding2genome", "no", "C4GPU_CODING2GENOME_SDP=2"): (("bsdp",), False),
    ("coding2coding", "yes", "none"): ((), False),
    ("coding2coding", "yes", "C4GPU_CODING2GENOME=1"): ((), False),
    ("coding2coding", "yes", "C4GPU_CODING2GENOME_SDP=1"): ((), False),
    ("coding2coding", "yes", "C4GPU_CODING2GENOME_BSDP=1"): ((), False),
    ("coding2coding", "yes", "C4GPU_CODON_SDP=1"): (("sdp",), False),
    ("coding2coding", "yes", "C4GPU_CODON_SEED=1"): (("hsp", "seed"), False),
    ("coding2coding", "yes", "C4GPU_CODING2GENOME_BSDP=2"): ((), False),
    ("coding2coding", "yes", "C4GPU_CODING2GENOME_SDP=2"): ((), False),
    ("coding2coding", "no", "none"): (("bsdp",), True),
    ("coding2coding", "no", "C4GPU_CODING2GENOME=1"): (("bsdp",), True),
    ("coding2coding", "no", "C4GPU_CODING2GENOME_SDP=1"): (("bsdp",), True),
    ("coding2coding", "no", "C4GPU_CODING2GENOME_BSDP=1"): (("bsdp",), True),
    ("coding2coding", "no", "C4GPU_CODON_SDP=1"): (("bsdp",), True),
    ("coding2coding", "no", "C4GPU_CODON_SEED=1"): (("bsdp", "hsp", "seed"), True),
    ("coding2coding", "no", "C4GPU_CODING2GENOME_BSDP=2"): (("bsdp",), True),
    ("coding2coding", "no", "C4GPU_CODING2GENOME_SDP=2"): (("bsdp",), True),
}


def bsdp_served(err):
    return re.search(r"c4gpu bsdp: \d+ pairs in \d+ flush", err) is not None


@functools.lru_cache(maxsize=None)
def reference(model, gapped, qf, tf):
    ref = subprocess.run([CPU_EXE, "-m", model, "--gappedextension", gapped] + REPORTS + [qf, tf],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    return ref.stdout


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("switch_matrix"), *inputs())


def run(exe, fasta, model, gapped, case):
    """(stdout, stderr) of one run of the drop-in binary `exe` under the case's switch."""
    env = dict(os.environ, C4GPU_VERBOSE="1", **HOST)
    for s in SWITCHES:
        env.pop(s, None)
    if case != "none":
        name, value = case.split("=")
        env[name] = value
    gpu = subprocess.run([exe, "-m", model, "--gappedextension", gapped] + REPORTS + list(fasta),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=env)
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return gpu.stdout, gpu.stderr.decode()


def seams_reporting(err):
    return tuple(s for s in SEAMS if "c4gpu %s:" % s in err)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gapped", ["yes", "no"])
@pytest.mark.parametrize("model", ["coding2genome", "coding2coding"])
def test_the_switch_opens_the_seams_it_opened_before(fasta, model, gapped, case):
    out, err = run(GPU_EXE, fasta, model, gapped, case)
    assert out == reference(model, gapped, *fasta)
    assert out.count(b"vulgar:") >= 3
    assert (seams_reporting(err), bsdp_served(err)) == EXPECTED[(model, gapped, case)], err[-1500:]


def test_a_switch_that_means_nonzero_serves_at_two(fasta):
    """C4GPU_CODING2GENOME_SDP: nonzero.  At 2 the SDP seam serves every pair it collects, as at 1."""
    for value in ("1", "2"):
        line = sdp_line(run(GPU_EXE, fasta, "coding2genome", "yes", "C4GPU_CODING2GENOME_SDP=" + value)[1])
        assert line and line[0] >= 3 and line[2] == line[0]
