"""The drop-in with C4GPU_SEED_BUILD=1 (integration/c4gpu_seed.c): step 1 of the word-scan seam builds the seeder's word table on
the device from the seeder's own queries (c4gpu_wordtab_build) instead of reading it off the reference's automaton.  The output
is the reference's byte for byte, with and without the fused route; C4GPU_SEED_BUILD_CHECK=1 also reads the automaton and finds
no word and no emission that differs; a seeder the switch does not take (a codon loader, --saturatethreshold) runs as before."""
import os
import random
import re
import subprocess

import pytest

from test_integration_bsdp_host import run_pair, GPU_EXE, CPU_EXE

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                 reason="reference binaries are built in the build container (make -C integration)")]

AA = "ARNDCQEGHILKMFPSTWYV"


def _protein_pair(tmp_path, extra, env_extra, n=6, seed=3):
    """affine:local on proteins: related protein sets (run_pair's inputs for that model are DNA)."""
    rng = random.Random(seed)
    aa = lambda k: "".join(rng.choice(AA) for _ in range(k))
    qf, tf = str(tmp_path / "qp.fa"), str(tmp_path / "tp.fa")
    with open(qf, "w") as fq, open(tf, "w") as ft:
        for k in range(n):
            q = aa(rng.randint(90, 200))
            t = aa(rng.randint(10, 80)) + "".join(rng.choice(AA) if rng.random() < 0.08 else c for c in q) + aa(rng.randint(10, 80))
            fq.write(">q%d\n%s\n" % (k, q))
            ft.write(">t%d\n%s\n" % (k, t))
    args = ["-m", "affine:local", "--showalignment", "yes", "--showvulgar", "yes", "-V", "0"] + list(extra) + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **env_extra))
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return ref.stdout, gpu.stdout, gpu.stderr.decode()


def _tables(err):
    m = re.search(r"c4gpu seed: word tables: (\d+) read off the automaton, (\d+) built on the device", err)
    assert m, err[-1500:]
    return int(m.group(1)), int(m.group(2))


CASES = [("protein2genome", ["--gappedextension", "yes"]),
         ("affine:local/protein", ["--gappedextension", "yes"]),
         ("est2genome", ["--gappedextension", "yes", "--dnawordlen", "8", "--dnawordlimit", "9"])]


def _run(tmp_path, model, extra, env):
    if model == "affine:local/protein":
        return _protein_pair(tmp_path, extra, env)
    return run_pair(tmp_path, model, extra, env, n=6, seed=43)


@pytest.mark.parametrize("fused", [False, True], ids=["scan", "fused"])
@pytest.mark.parametrize("model,extra", CASES, ids=[c[0] for c in CASES])
def test_built_table_is_the_automatons_and_the_output_the_references(tmp_path, model, extra, fused):
    env = {"C4GPU_SEED_BUILD": "1", "C4GPU_SEED_BUILD_CHECK": "1", "C4GPU_SEED_FACTOR": "0"}
    if fused:
        env["C4GPU_SEED_FUSED"] = "1"
    ref, gpu, err = _run(tmp_path, model, extra, env)
    assert gpu == ref and ref.count(b"vulgar:") >= 3
    checks = re.findall(r"c4gpu seed: build check (\d+) words, (\d+) mismatches", err)
    assert checks and all(int(w) > 0 and int(m) == 0 for w, m in checks), err[-1500:]
    read, built = _tables(err)
    assert built == len(checks) == read                       # (the check reads every automaton too)
    assert "is read off the automaton" not in err and "scanned on the CPU" not in err
    if fused:
        m = re.search(r"c4gpu seed fused: (\d+) targets through c4gpu_seed_extend: (\d+) word hits", err)
        assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, err[-1500:]
        assert "takes the scan and extension calls" not in err


@pytest.mark.parametrize("fused", [False, True], ids=["scan", "fused"])
def test_without_the_check_no_automaton_is_read(tmp_path, fused):
    env = {"C4GPU_SEED_BUILD": "1", "C4GPU_SEED_FACTOR": "0"}
    if fused:
        env["C4GPU_SEED_FUSED"] = "1"
    ref, gpu, err = run_pair(tmp_path, "protein2genome", ["--gappedextension", "yes"], env, n=6, seed=43)
    assert gpu == ref and ref.count(b"vulgar:") >= 3
    assert _tables(err)[0] == 0 and _tables(err)[1] > 0
    assert "build check" not in err


def test_seeders_the_switch_does_not_take(tmp_path):
    """A codon loader: the table is read off the automaton as before.  --saturatethreshold: the seeder keeps the reference's
    walk altogether (no table of either kind)."""
    env = {"C4GPU_SEED_BUILD": "1", "C4GPU_SEED_FACTOR": "0", "C4GPU_CODON_SEED": "1"}
    ref, gpu, err = run_pair(tmp_path, "coding2coding", ["--gappedextension", "yes"], env, n=4, seed=44)
    assert gpu == ref
    read, built = _tables(err)
    assert read > 0 and built == 0
    ref, gpu, err = run_pair(tmp_path, "affine:local", ["--gappedextension", "yes", "--saturatethreshold", "20"],
                             {"C4GPU_SEED_BUILD": "1", "C4GPU_SEED_FACTOR": "0"}, n=4, seed=45)
    assert gpu == ref
    assert "built on the device" not in err and "build check" not in err
