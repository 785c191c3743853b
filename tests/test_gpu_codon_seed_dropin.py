"""The opt-in codon seeding of the drop-in binary (C4GPU_CODON_SEED=1) with the device doing the work: heuristic ungapped:trans
and coding2coding runs whose word scan (c4gpu_seed_scan) and HSP extensions (c4gpu_hsp_extend_chains / _chains_masked with
C4GPU_MATCH_CODON2CODON) -- or, fused, the one c4gpu_seed_extend call per target -- come from the library; the output is the
reference's, byte for byte.  Once more with every seed and every extension compared with the reference's own functions inside
the run.  The seams' host modes: test_codon_seed_dropin_host.py."""
import os

import pytest

from test_codon_seed_dropin_host import RUNS, run, seed_line, GPU_EXE, CPU_EXE
from test_softmask_dropin_host import hsp_line
from test_integration_seed_fused_host import fused_line

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                 reason="reference binaries are built in the build container (make -C integration)")]

DEVICE = {"C4GPU_CODON_SEED": "1", "C4GPU_SEED_FACTOR": "0", "C4GPU_BATCH": "4096"}
NAMES = ["trans", "trans_softmaskboth", "coding2coding_sdp", "coding2coding_bsdp"]


@pytest.mark.parametrize("name", NAMES)
def test_runs_on_the_device_are_byte_identical(tmp_path, name):
    ref, gpu, err = run(tmp_path, name, DEVICE)
    assert gpu == ref and ref.count(b"vulgar:") >= 6
    line = hsp_line(err)
    assert line["hits"] > 200 and line["stored"] > 0
    if RUNS[name][1]:
        assert line["dropped"] > 0, err[-600:]
    assert seed_line(err)[0] > 0
    assert "HSP extensions of this scan on the CPU" not in err and "scanned on the CPU" not in err


@pytest.mark.parametrize("name", NAMES)
def test_every_seed_and_every_extension_checked_inside_the_run(tmp_path, name):
    ref, gpu, err = run(tmp_path, name, dict(DEVICE, C4GPU_HSP_CHECK="1", C4GPU_SEED_CHECK="1"))
    assert gpu == ref
    assert hsp_line(err)["checked"] > 0
    assert "every seed equal to the reference's own walk" in err


@pytest.mark.parametrize("name", ["trans", "coding2coding_sdp", "coding2coding_bsdp"])
def test_fused_route_on_the_device_is_byte_identical(tmp_path, name):
    ref, gpu, err = run(tmp_path, name, dict(DEVICE, C4GPU_SEED_FUSED="1"))
    assert gpu == ref and ref.count(b"vulgar:") >= 6
    targets, hits, extended, kept = fused_line(err)
    assert targets > 0 and hits > 200 and hits > extended >= kept > 0
    assert "takes the scan and extension calls" not in err and "scanned on the CPU" not in err
    assert "c4gpu hsp:" not in err                      # no word hit went through the extension seam
