"""BSDP's derived models of coding2coding (start terminal, end terminal, join of match state 2) and the heuristic runs that use
them: the vector sets of tools/make_codon_derived_golden.py (made by the reference's refdump --derived), their models, and the
inputs and the runner of the drop-in checks; shared by tests/test_codon_derived.py (no device) and
tests/test_gpu_codon_derived.py.  Data and plumbing only; no reference code."""
import functools, os, random, re, subprocess

import exonerate_amd as ex
from exonerate_amd import _abi
import oracle_lib
import codon_cases as cc
from golden_util import apply_flags, load_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_EXE = os.path.join(ROOT, "integration", "_build", "exonerate-gpu")
CPU_EXE = os.path.join(ROOT, "oracle", "_ref", "exonerate-compiled")
HAVE_BINARIES = os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)

ALT_FLAGS = ["--codongapopen", "-11", "--codongapextend", "-3", "--frameshift", "-13"]
# role -> (src state, dst state, start scope, end scope)
ROLES = {"start": (0, 2, 0, 4), "end": (2, 1, 4, 0), "join": (2, 2, 4, 4)}
SETS = ["derived_coding2coding%s_%s" % (tag, role) for tag in ("", "_codonalt") for role in ("start", "end", "join")]
# what the reference calls them (C4_DerivedModel_create, c4.c: Segment("src"->"dst"):[original])
REF_NAME = {"start": 'Segment("START"->"match"):[coding2coding]', "end": 'Segment("match"->"END"):[coding2coding]',
            "join": 'Segment("match"->"match"):[coding2coding]'}
ROWS_PER_LANE = 3                       # the derived codon kernels (tools/gen_kernel_tus.py); a strip is 64 x 3 query rows


def set_role(name):
    return name.rsplit("_", 1)[1]


def set_params(name):
    return apply_flags(ex.default_params(), ALT_FLAGS if "_codonalt" in name else [])


def set_model(name):
    return ex.Model.derived("coding2coding", *ROLES[set_role(name)], params=set_params(name))


@functools.lru_cache(maxsize=None)
def records(name):
    return tuple(load_set(name))


def expected(rec):
    """(score, region, ops) of a record; a record without a path: (score, None, None)."""
    if "path_score" not in rec:
        return rec["score"], None, None
    return rec["path_score"], tuple(rec["region"]), [tuple(o) for o in rec["ops"]]


def of_result(g):
    """The same triple of an Engine.viterbi / ResidentBatch.viterbi result (ops: (transition, run length), START -> END)."""
    region = (g["query_start"], g["target_start"], g["query_end"] - g["query_start"], g["target_end"] - g["target_start"])
    return g["score"], region, runs(g["ops"])


def runs(ops):
    out = []
    for tr in ops:
        if out and out[-1][0] == tr:
            out[-1] = (tr, out[-1][1] + 1)
        else:
            out.append((tr, 1))
    return out


def oracle(model, mode, q, t, region):
    """oracle_viterbi on one rectangle: (score, region, ops as runs)."""
    olib = oracle_lib.load()
    vo = oracle_lib.ViterbiOut()
    olib.oracle_viterbi(model.c, model.params, mode, q.encode(), len(q), t.encode(), len(t), _abi.Region(*region), None, 0, vo)
    out = (vo.score, (vo.query_start, vo.target_start, vo.query_end - vo.query_start, vo.target_end - vo.target_start),
           runs([vo.ops[x] for x in range(vo.n_ops)]))
    olib.oracle_viterbi_out_clear(vo)
    return out


# ---- the heuristic runs ------------------------------------------------------------------------------------------------
def coding_pairs(n=8, seed=77):
    """n homologous coding pairs, queries of 400 to 800 bases: synonymous codons drawn apart, a tenth of the residues replaced,
    and three planted events each (one- and two-base frameshifts and one to three whole codons, on either axis) far enough apart
    that HSPs grow between them; the target carries random flanks."""
    rng = random.Random(seed)
    qs, ts = [], []
    for k in range(n):
        ncod = rng.randint(134, 260)
        qc, tc = cc._homologous(rng, [rng.choice(cc.AA) for _ in range(ncod)], 0.08)
        kinds = [("q1", "t2", "qc"), ("t1", "q2", "tc"), ("q2", "tc", "t1"), ("qc", "q1", "t2")][k % 4]
        for slot, kind in enumerate(kinds):
            at = ncod * (slot + 1) // 4 + rng.randint(-6, 6)
            side = qc if kind[0] == "q" else tc
            if kind[1] == "c":
                side[at:at] = [rng.choice(cc.CODONS[rng.choice(cc.AA)]) for _ in range(rng.randint(1, 3))]
            else:
                side[at] += cc._dna(rng, int(kind[1]))
        q = "".join(qc)[:800]
        t = cc._dna(rng, rng.randint(30, 120)) + "".join(tc) + cc._dna(rng, rng.randint(30, 120))
        qs.append(("cq%d" % k, q))
        ts.append(("ct%d" % k, t))
    return qs, ts


def run_pair(tmp_path, model, extra, env_extra, inputs=None, ref=True):
    """(reference stdout or None, drop-in stdout, drop-in stderr) of a BSDP-mode run (--gappedextension no) on `inputs`
    (default: coding_pairs())."""
    qs, ts = inputs or coding_pairs()
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    for path, recs in ((qf, qs), (tf, ts)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(">%s\n%s\n" % (name, seq))
    args = ["-m", model, "--gappedextension", "no", "--showalignment", "yes", "--showvulgar", "yes", "-V", "0"] + list(extra) + [qf, tf]
    rp = subprocess.Popen([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE) if ref else None
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **env_extra))
    ref_out = None
    if rp:
        ref_out, ref_err = rp.communicate(timeout=600)
        assert rp.returncode == 0, ref_err.decode()[-800:]
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return ref_out, gpu.stdout, gpu.stderr.decode()


def served(err):
    """(score calls served, score calls, path calls served, path calls) of the seam's report line; None: no such line."""
    m = re.search(r"(\d+) of (\d+) score calls and (\d+) of (\d+) path calls served", err)
    return [int(x) for x in m.groups()] if m else None


def refinements(err):
    m = re.search(r"(\d+) of (\d+) refinements from refinement batches", err)
    return (int(m.group(1)), int(m.group(2))) if m else None
