"""Soft-masked runs through the drop-in binary with the device doing the work: the HSP sets of --softmasktarget /
--softmaskquery runs are extended by c4gpu_hsp_extend_chains_masked (hspset.c:981-995), every seed's result is compared with
the reference's own HSPset_seed_hsp (C4GPU_HSP_CHECK=1: the run aborts at the first difference), and stdout is byte-identical
to the unmodified reference's.  The same cases on the host modes of the seams: test_softmask_dropin_host.py."""
import os
import pytest

from test_integration_bsdp_host import GPU_EXE, CPU_EXE
from test_softmask_dropin_host import run_softmask, hsp_line

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                 reason="reference binaries are built in the build container (make -C integration)")]


@pytest.mark.parametrize("model,mask,gapped", [("est2genome", "target", "no"), ("protein2genome", "both", "yes"),
                                               ("affine:local", "query", "yes")])
def test_softmasked_runs_on_the_device_are_byte_identical(tmp_path, model, mask, gapped):
    ref, gpu, err = run_softmask(tmp_path, {"C4GPU_HSP_CHECK": "1"}, model, gapped, mask)
    assert gpu == ref and ref.count(b"vulgar:") >= 2
    line = hsp_line(err)
    # extended on the device (the host mode checks nothing: it IS the reference's function), seeds dropped at masked ends
    assert line["hits"] > 50 and line["batches"] >= 1 and line["checked"] > 0 and line["stored"] > 0
    if mask != "query":
        assert line["dropped"] > 0, err[-600:]
    assert "HSP extensions of this scan on the CPU" not in err
