"""BSDP's derived models of coding2genome -- the terminals and the join of match state 2, and the span src / dst models of its three
intron phases (span states 11, 12, 13) -- and the heuristic runs that use them: the vector sets of
tools/make_coding2genome_derived_golden.py (made by the reference's refdump), their models, what the sets were selected to cover,
refdump run on the spot, and the inputs and the runner of the drop-in checks.  Shared by tests/test_coding2genome_derived.py (no
device) and tests/test_gpu_coding2genome_derived.py.  Data and plumbing only; no reference code."""
import functools, json, os, random, subprocess, tempfile

import exonerate_amd as ex
from exonerate_amd import _abi
import coding2genome_cases as cg
from codon_derived_cases import run_pair, served, refinements, runs, of_result, expected, HAVE_BINARIES   # noqa: F401
from golden_util import GOLDEN_DIR, apply_flags, load_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
HAVE_REFDUMP = os.path.exists(REFDUMP)

# the non-default parameter point: codon gap and frameshift penalties, the intron penalty and the intron length limits
ALT_FLAGS = ["--codongapopen", "-11", "--codongapextend", "-3", "--frameshift", "-13", "--intronpenalty", "-22",
             "--minintron", "24", "--maxintron", "60"]
# role -> (src state, dst state, start scope, end scope): C4_DerivedModel_create on match state 2 (heuristic.c:242-330)
ROLES = {"start": (0, 2, 0, 4), "end": (2, 1, 4, 0), "join": (2, 2, 4, 4)}
SPAN_STATE = {0: 11, 1: 12, 2: 13}      # intron 0:0, 1:2, 2:1
SETS = ["derived_coding2genome%s_%s" % (tag, role) for tag in ("", "_alt") for role in ("start", "end", "join")]
SPAN_SETS = ["span_coding2genome_phase%d" % ph for ph in range(3)]
CLI_SET = "codon_cli_coding2genome_bsdp"
REF_NAME = {"start": 'Segment("START"->"match"):[coding2genome]', "end": 'Segment("match"->"END"):[coding2genome]',
            "join": 'Segment("match"->"match"):[coding2genome]'}
ROWS_PER_LANE = 3                       # tools/gen_kernel_tus.py: DERIVED_R["coding2genome"]
STRIP = 64 * ROWS_PER_LANE              # query rows (0 ... Q) one strip holds
SMALL, MAX_Q, MAX_T = 49, 210, 120


def span_src(phase, params=None, traceback=False):
    """match -> span state, CORNER / ANYWHERE (cell_end_func); traceback: the CORNER / CORNER model of the same tables."""
    return ex.Model.derived("coding2genome", 2, SPAN_STATE[phase], 4, 4 if traceback else 0, params=params)


def span_dst(phase, params=None):
    return ex.Model.derived("coding2genome", SPAN_STATE[phase], 2, 0, 4, params=params)


def all_models():
    """name -> the nine derived models (the src traceback model shares the src tables)."""
    out = {role: ex.Model.derived("coding2genome", *spec) for role, spec in ROLES.items()}
    for ph in range(3):
        out["phase%d_span_src" % ph] = span_src(ph)
        out["phase%d_span_dst" % ph] = span_dst(ph)
    return out


def set_role(name):
    return name.rsplit("_", 1)[1]


def set_params(name):
    return apply_flags(ex.default_params(), ALT_FLAGS if "_alt_" in name else [])


def set_model(name):
    return ex.Model.derived("coding2genome", *ROLES[set_role(name)], params=set_params(name))


@functools.lru_cache(maxsize=None)
def records(name):
    return tuple(load_set(name))


def load_cli():
    with open(os.path.join(GOLDEN_DIR, CLI_SET + ".json")) as f:
        return json.load(f)


# ---- what a set covers -------------------------------------------------------------------------------------------------
def is_small(rec):
    """At most 49 x 49 plus the intron(s) of its path."""
    intron = sum(n for _, _, n in rec.get("_introns", ()))
    return len(rec["query"]) <= SMALL and len(rec["target"]) - intron <= SMALL


def features(model, rec):
    """What the reference's path of this record shows, read off the derived table's transitions."""
    f = {"q%d" % (len(rec["query"]) % 3) + "t%d" % (len(rec["target"]) % 3)}
    rec["_introns"] = ()
    if "path_score" not in rec or not rec["ops"]:
        return f
    rec["_introns"] = tuple(cg.introns_of(model, rec["ops"], rec["region"]))
    for ph, _, _ in rec["_introns"]:
        f.add("intron%d" % ph)
    trs = [model.c.transitions[tr] for tr, _ in rec["ops"]]
    for t in trs:
        name = t.name.decode()
        if name.startswith("frameshift open"):
            f.add("qshift" if t.advance_query else "tshift")
        if name in ("insert", "match to insert"):
            f.add("insert")
        if name in ("delete", "match to delete"):
            f.add("delete")
    if trs[0].name.decode() != "match":
        f.add("begins_off_match")
    if trs[-1].name.decode() != "match":
        f.add("ends_off_match")
    return f


def needs(role):
    """[(predicate on (record, features), records asked)] of a set of this role."""
    n = [(lambda r, f: len(r["query"]) == 1, 1), (lambda r, f: len(r["query"]) == 2, 1),
         (lambda r, f: len(r["target"]) == 1, 1), (lambda r, f: len(r["target"]) == 2, 1),
         (lambda r, f: len(r["query"]) + 1 == STRIP - 1 and "path_score" in r, 1),
         (lambda r, f: len(r["query"]) + 1 == STRIP + 1 and "path_score" in r, 1)]
    if role == "join":
        n += [(lambda r, f, k="q%dt%d" % (a, b): k in f, 1) for a in range(3) for b in range(3)]
        n += [(lambda r, f, k="intron%d" % ph: k in f, 3) for ph in range(3)]
        n += [(lambda r, f, k=k: k in f, 1) for k in ("qshift", "tshift", "insert", "delete")]
    else:
        key = "ends_off_match" if role == "start" else "begins_off_match"
        n += [(lambda r, f: key in f and any(k.startswith("intron") for k in f), 1), (lambda r, f: key in f, 4)]
    return n


def check_set(model, recs, role):
    """The requirements of a derived set, on its records (the generator refuses to write a set that fails; the tests hold the
    committed files to the same)."""
    assert 0 < len(recs) <= 40, len(recs)
    feats = [features(model, r) for r in recs]
    assert all(len(r["query"]) <= MAX_Q and len(r["target"]) <= MAX_T for r in recs)
    assert 4 * sum(1 for r in recs if is_small(r)) >= 3 * len(recs), role
    for n, (pred, count) in enumerate(needs(role)):
        have = sum(1 for r, f in zip(recs, feats) if pred(r, f))
        assert have >= count, "set %s: requirement %d holds for %d records, %d asked" % (role, n, have, count)
    for r in recs:
        r.pop("_introns", None)


def walk(model, rec):
    """The recorded ops chained through the model's table from START to END: (query advance, target advance).  (A span dst path
    starts inside an open intron, whose start lies in the start cell: coding2genome_cases.replay's length test has no shadow.)"""
    m = model.c
    state, dq, dt = m.start_state, 0, 0
    for tr, length in rec["ops"]:
        d = m.transitions[tr]
        for _ in range(length):
            assert d.input == state, (rec["id"], tr, state)
            state = d.output
        dq += d.advance_query * length
        dt += d.advance_target * length
    assert state == m.end_state, rec["id"]
    return dq, dt


def span_usable(rec):
    return bool(rec.get("end_cells")) and rec.get("dst_score", _abi.IMPOSSIBLY_LOW_SCORE) > _abi.IMPOSSIBLY_LOW_SCORE and \
        "path_score" in rec and bool(rec.get("ops"))


def span_post_row(dst, rec):
    """The query row (of the rectangle) in which the dst path's split-codon post transition ends; None: no such transition."""
    i = rec["region"][0]
    for tr, length in rec["ops"]:
        d = dst.c.transitions[tr]
        i += d.advance_query * length
        if d.name.decode().startswith(("phase1post", "phase2post")):
            return i
    return None


def span_two_lanes(rec):
    """END cells in the rows of two different lanes: query rows on both sides of a multiple of ROWS_PER_LANE."""
    return len({c[0] // ROWS_PER_LANE for c in rec["end_cells"]}) >= 2


def check_span_set(dst, recs, phase):
    assert 8 <= len(recs) <= 10, len(recs)
    assert all(span_usable(r) for r in recs)
    assert sum(len(json.dumps(r, separators=(",", ":"))) + 1 for r in recs) <= 100000
    if phase:
        early = [r for r in recs if span_post_row(dst, r) is not None and span_post_row(dst, r) <= 3]
        assert len(early) >= 2, (phase, len(early))
    assert any(span_two_lanes(r) for r in recs)
    assert any(len(r["query"]) + 1 >= 8 * ROWS_PER_LANE for r in recs)          # one rectangle of eight lanes or more


# ---- refdump on the spot -----------------------------------------------------------------------------------------------
def _refdump(args, cases):
    out = []
    for k in range(0, len(cases), 16):
        with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as f:
            for c in cases[k:k + 16]:
                f.write("%s\t%s\t%s\n" % c)
            path = f.name
        try:
            r = subprocess.run([REFDUMP] + args + ["--input", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        finally:
            os.unlink(path)
        out += [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert [r["id"] for r in out] == [c[0] for c in cases]
    for r, c in zip(out, cases):
        r["query"], r["target"] = c[1], c[2]
    return out


def refdump_derived(role, cases, flags=()):
    """The reference's Optimal_find_score / find_path of a derived model on whole pairs: records like the sets'."""
    return _refdump(["--cmd", "golden", "--model", "coding2genome", "-D", "32", "--derived", "%d,%d,%d,%d" % ROLES[role]] + list(flags),
                    cases)


def refdump_span(phase, cases):
    return _refdump(["--cmd", "span", "--model", "coding2genome", "--derived", "2,%d" % SPAN_STATE[phase]], cases)


# ---- generated pairs ---------------------------------------------------------------------------------------------------
EDGE_ROWS = (2, 3, 191, 192, 193)
EDGE_WHAT = ("split", "exit", "shift")
EDGE_SEED = 7117                 # checked with refdump: every edge pair's join path holds the planted phase's intron and the event on its row


def edge_pair(rng, row, phase, what):
    """A whole small pair in which `what` sits on query row `row` of the rectangle: "split" = the first row of the codon the intron
    of `phase` splits (phase 0: the row of the 5' exit), "exit" = the row of the 3' exit (`phase` rows further down), "shift" = the
    cell a frameshift opens into, four codons in front of the intron: row % 3 extra query bases behind row // 3 matched codons
    (rows 2, 191, 193: the path leaves the corner, or the codon above, with a query frameshift) or, where row % 3 == 0, one extra
    target base in that row.  The codons are the same on both sides; the target holds one intron of 30 to 40 bases."""
    if what == "shift":
        ci = row // 3
        kind = "q%d" % (row % 3) if row % 3 else "t1"
        return cg.gene_pair(rng, ci + 12, introns=[(ci + 4, phase, rng.randint(30, 40))], events=[(kind, ci)], flank_t=0, sub=0.0)
    first = row - phase if what == "exit" else row
    flank, ci = first % 3, first // 3
    return cg.gene_pair(rng, ci + 8, introns=[(ci, phase, rng.randint(30, 40))], flank_q=flank, flank_t=0, sub=0.0)


def edge_cases():
    rng = random.Random(EDGE_SEED)
    return [("e%d_%d_%s" % (row, phase, what), ) + edge_pair(rng, row, phase, what)
            for row in EDGE_ROWS for phase in range(3) for what in EDGE_WHAT]


def event_rows(model, rec):
    """{(what, query row of the rectangle)} of a recorded path: where a split codon starts ("split", with the phase), where the
    3' exit leaves ("exit") and the row of the cell a frameshift (on either axis) opens into ("shift")."""
    out, i = set(), rec["region"][0]
    for tr, length in rec["ops"]:
        d = model.c.transitions[tr]
        name = d.name.decode()
        if name.startswith("(START) to phase") or name.startswith("(START) to intron 0:0"):
            out.add(("split", i))
        if d.label == _abi.LABEL_3SS:
            out.add(("exit", i))
        if name.startswith("frameshift open"):
            out.add(("shift", i + d.advance_query))
        i += d.advance_query * length
    return out


FUZZ_SEED = 30303                # checked with refdump: the join paths of the 60 pairs hold each phase's intron at least twice


def fuzz_pair(rng):
    """A BSDP-sized whole pair: 1 to 16 codons, most with an intron of 30 to 50 bases at any phase, events, flanks."""
    n_aa = rng.randint(1, 16)
    introns = [(rng.randint(2, n_aa - 3), rng.randrange(3), rng.randint(30, 50))] if n_aa >= 6 and rng.random() < 0.7 else []
    events = [(rng.choice(("q1", "q2", "qc", "t1", "t2", "tc")), rng.randrange(n_aa))] if rng.random() < 0.4 else []
    q, t = cg.gene_pair(rng, n_aa, introns=introns, events=events, flank_q=rng.choice((0, 0, 1, 2)), flank_t=rng.choice((0, 0, 1, 3)),
                        sub=0.05, keep=2)
    return q[:SMALL], t[:MAX_T]


# ---- the heuristic runs ------------------------------------------------------------------------------------------------
CLI_VARIANTS = {"default": [], "S_no": ["-S", "no"], "refine_region": ["--refine", "region"],
                "refine_full_bestn1": ["--refine", "full", "--bestn", "1"]}
CLI_REPORTS = ["--showtargetgff", "yes"]          # beside run_pair's --showvulgar yes --showalignment yes


def stable_lines(stdout):
    """A run's stdout without the lines that name the command, the host and the date."""
    return [l for l in stdout.decode().split("\n") if not l.startswith(("Command line:", "Hostname:", "##date "))]


def cli_stdout(data, variant):
    """The recorded lines of a variant (a variant whose output equals an earlier one's is stored as that one's name)."""
    out = data["variants"][variant]["stdout"]
    return data["variants"][out]["stdout"] if isinstance(out, str) else out


def check_cli(data):
    """What the recorded runs show: introns of all three phases (vulgar: a phase-0 intron follows a codon run directly, a phase-1
    intron a split codon `S 1 1`, a phase-2 intron `S 2 2`), an alignment with two introns, both target strands."""
    vulgar = [l.split() for l in cli_stdout(data, "default") if l.startswith("vulgar:")]
    phases = set()
    for v in vulgar:
        ops = [tuple(v[k:k + 3]) for k in range(10, len(v), 3)]
        for k, op in enumerate(ops):
            if op[0] == "5":
                phases.add(int(ops[k - 1][1]) if ops[k - 1][0] == "S" else 0)
    assert phases == {0, 1, 2}, phases
    assert any(sum(1 for k in range(10, len(v), 3) if v[k] == "I") >= 2 for v in vulgar)
    assert {v[8] for v in vulgar} == {"+", "-"}
    for name, flags in CLI_VARIANTS.items():
        assert data["variants"][name]["flags"] == flags and any(l.startswith("vulgar:") for l in cli_stdout(data, name)), name


def cli_inputs(seed=4242):
    """Three CDS queries against three genomic windows: exons of 28 to 36 codons (long enough to seed HSPs) around introns of all
    three phases, one gene with two introns, one window on the minus strand."""
    rng = random.Random(seed)
    shapes = [[(30, 0, 70)], [(32, 1, 85)], [(30, 1, 90), (62, 2, 72)]]
    qs, ts = [], []
    for k, introns in enumerate(shapes):
        n_aa = introns[-1][0] + rng.randint(28, 36)
        q, t = cg.gene_pair(rng, n_aa, introns=introns, flank_t=None, sub=0.05, keep=3)
        t = cg.dna(rng, rng.randint(30, 60)) + t + cg.dna(rng, rng.randint(30, 60))
        if k == 1:
            t = cg.revcomp(t)
        qs.append(("cds%d" % k, q))
        ts.append(("win%d" % k, t))
    return qs, ts
