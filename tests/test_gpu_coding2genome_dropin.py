"""`exonerate-gpu --model coding2genome --exhaustive yes` (the reference's own binary with integration/c4gpu_shim.c linked in) on
the FASTA pairs of the recorded CLI set (tests/golden/codon_cli_coding2genome.json): with C4GPU_CODING2GENOME=1 the device family
serves the run and stdout is the recorded one byte for byte; without the variable the run is the reference's own, the same bytes,
and no kernel of the family is launched.  The binary is built in the build container and travels with the repo."""
import os, re, subprocess

import pytest

from coding2genome_cases import load_cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_EXE = os.path.join(ROOT, "integration", "_build", "exonerate-gpu")
needs_binary = pytest.mark.skipif(not os.path.exists(GPU_EXE), reason="exonerate-gpu is built in the build container (make -C integration)")


def _run(tmp_path, pair, reports, env):
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    with open(qf, "w") as f:
        f.write(">%s %s\n%s\n" % (pair["id"], pair["qdef"], pair["query"]))
    with open(tf, "w") as f:
        f.write(">%s\n%s\n" % (pair["tid"], pair["target"]))
    r = subprocess.run([GPU_EXE, "--model", "coding2genome", "--exhaustive", "yes"] + reports + [qf, tf], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, C4GPU_TRACE="1", C4GPU_MIN_CELLS="0", **env))
    err = r.stderr.decode()
    assert r.returncode == 0, err[-2000:]
    # the recording dropped the lines that name the command, the host and the day
    out = "\n".join(l for l in r.stdout.decode().split("\n") if not l.startswith(("Command line:", "Hostname:", "##date ")))
    return out, re.findall(r"c4gpu trace:   kernel (k\w+):", err)


@needs_binary
@pytest.mark.parametrize("k", [0, 1])
def test_with_the_variable_the_device_serves_the_run(tmp_path, k):
    data = load_cli()
    pair = data["pairs"][k]
    out, kernels = _run(tmp_path, pair, data["reports"], {"C4GPU_CODING2GENOME": "1"})
    assert out == "\n".join(pair["stdout"]), pair["id"]
    assert kernels and all("_coding2genome_" in x for x in kernels), kernels


@needs_binary
@pytest.mark.parametrize("k", [0, 1])
def test_without_the_variable_the_run_is_the_reference_s(tmp_path, k):
    data = load_cli()
    pair = data["pairs"][k]
    env = {x: v for x, v in os.environ.items() if x != "C4GPU_CODING2GENOME"}
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    with open(qf, "w") as f:
        f.write(">%s %s\n%s\n" % (pair["id"], pair["qdef"], pair["query"]))
    with open(tf, "w") as f:
        f.write(">%s\n%s\n" % (pair["tid"], pair["target"]))
    r = subprocess.run([GPU_EXE, "--model", "coding2genome", "--exhaustive", "yes"] + data["reports"] + [qf, tf], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600, env=dict(env, C4GPU_TRACE="1", C4GPU_MIN_CELLS="0"))
    err = r.stderr.decode()
    assert r.returncode == 0, err[-2000:]
    out = "\n".join(l for l in r.stdout.decode().split("\n") if not l.startswith(("Command line:", "Hostname:", "##date ")))
    assert out == "\n".join(pair["stdout"]), pair["id"]
    assert not re.findall(r"c4gpu trace:   kernel (k\w+):", err), err[-1500:]
