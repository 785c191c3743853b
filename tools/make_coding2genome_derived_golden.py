#!/usr/bin/env python3
"""Generate the vectors of BSDP's derived models of coding2genome under tests/golden/, by running the REFERENCE ITSELF
(`oracle/_ref/refdump --cmd golden --derived` and `--cmd span --derived`) on whole rectangles.  Runs only where the reference
binaries are built; tools/make_golden.py and every existing set are left alone.

  derived_coding2genome_{start,end,join}.jsonl        the terminals and the join of match state 2, default parameters
  derived_coding2genome_alt_{start,end,join}.jsonl    the same at ALT_FLAGS (codon gap, frameshift and intron penalties, intron
                                                      length limits)
  span_coding2genome_phase{0,1,2}.jsonl               src DP (END cells out) and dst DP (START cells in) of the span of each
                                                      intron phase (span states 11, 12, 13), in the shape of
                                                      span_protein2genome_phase*.jsonl
  codon_cli_coding2genome_bsdp.json                   stdout of the reference binary, --model coding2genome --gappedextension no,
                                                      on a handful of CDS against genomic windows: default, -S no,
                                                      --refine region, --refine full --bestn 1

Inputs are CDS / gene pairs of tests/coding2genome_cases.py (gene_pair: planted introns of every phase, one- and two-base
frameshifts, codon inserts and deletes), rectangles with a side of one or two bases and rectangles around the height of one strip
of the derived kernels (64 lanes x 3 rows).  A pool of candidates goes through the reference once per set; what is written is a
selection of at most 24 records, chosen -- and then asserted, the script refuses to write otherwise -- on the reference's own
operation lists (needs(), span_check()).  Every path record replays through the builder's tables first: region, advances and,
with the splice values the reference reports at the path's sites (rec["ss"]), the score.

Not met, and why: a span record with Q + 1 > 192 rows.  A span src DP sets END in nearly every cell right of the first 5' site, so
such a record alone lists more END cells than a 100 KB file holds; the device tests run those rectangles against refdump on the
spot instead (tests/test_gpu_coding2genome_derived.py)."""
import json, os, random, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exonerate_amd as ex                                          # noqa: E402
import coding2genome_cases as cg                                    # noqa: E402
import coding2genome_derived_cases as cd                            # noqa: E402
from golden_util import apply_flags                                 # noqa: E402

REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
OUT = os.path.join(ROOT, "tests", "golden")
MAX_RECORDS, MAX_Q, MAX_T, SMALL = 24, 210, 120, 49
STRIP = cd.STRIP


def pool(rng):
    out = []
    ev_kinds = ("q1", "q2", "qc", "t1", "t2", "tc")
    for k in range(260):                                            # BSDP-sized: up to 16 codons, an intron in most
        n_aa = rng.randint(3, 16)
        introns = []
        if n_aa >= 7 and k % 4:
            introns = [(rng.randint(3, n_aa - 3), k % 3, rng.randint(30, 64))]
        events = []
        if n_aa >= 8 and rng.random() < 0.5:
            events = [(rng.choice(ev_kinds), rng.choice([1, 2, n_aa - 2]))]
        q, t = cg.gene_pair(rng, n_aa, introns=introns, events=events, flank_q=rng.choice((0, 0, 1, 2)),
                            flank_t=rng.choice((0, 0, 1, 2, 4)), sub=0.04, keep=2)
        if k % 9 == 0 and introns:                                  # a terminal that stops inside or right behind the intron
            cut = t.find("GTAAGT") + rng.choice((2, 10, len(t)))
            t = t[:max(1, cut)]
        out.append((q[:SMALL], t[:MAX_T]))
    for k in range(12):                                             # two introns in one join
        q, t = cg.gene_pair(rng, 14, introns=[(4, k % 3, 30), (10, (k + 1) % 3, 31)], flank_t=0, sub=0.0, keep=2)
        out.append((q[:SMALL], t[:MAX_T]))
    for ql, tl in ((1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (2, 3), (3, 2), (1, 7), (7, 1), (2, 8), (8, 2), (1, 40),
                   (12, 2), (2, 50), (31, 1)):                      # a side of one or two bases
        q, t = cg.gene_pair(rng, max(ql, tl) // 3 + 1, flank_t=0, sub=0.0)
        out.append((q[:ql], t[:tl]))
    for ql in (STRIP - 2, STRIP - 1, STRIP, STRIP + 1, STRIP - 2, STRIP, STRIP - 2, STRIP):      # Q + 1 rows = 191 ... 194
        # the gene's last exons against the whole CDS: a long codon insert in the query, then an intron near the strip's last rows
        n_aa = ql // 3
        q, t = cg.query_of_length(rng, ql, introns=[(n_aa - rng.randint(3, 6), rng.randrange(3), rng.randint(30, 44))], flank_t=0,
                                  sub=0.02, keep=3)
        head = 3 * rng.randint(3, 6)
        t = t[:head] + t[len(t) - (MAX_T - head):]                  # the target keeps the first codons and the tail with the intron
        out.append((q, t))
    return [("cg%03d" % k, q, t) for k, (q, t) in enumerate(out) if q and t]


def thin_splice(model, rec):
    """Keeps of the splice arrays only the forward values at the first target position of the path's site transitions."""
    ss = {"5": {}, "3": {}}
    if "path_score" in rec:
        j = rec["region"][1]
        for tr, length in rec["ops"]:
            t = model.c.transitions[tr]
            if t.label == cg._abi.LABEL_5SS:
                ss["5"][str(j)] = rec["ss5_forward"][j]
            if t.label == cg._abi.LABEL_3SS:
                ss["3"][str(j)] = rec["ss3_forward"][j]
            j += t.advance_target * length
    for k in ("ss5_forward", "ss3_forward", "ss5_reverse", "ss3_reverse", "sugar", "cigar", "vulgar", "qlen", "tlen"):
        rec.pop(k, None)                                            # (the printers are not these sets' business)
    rec["ss"] = ss


def select(recs, feats, role, rng):
    chosen = []
    for pred, count in cd.needs(role):
        have = sum(1 for k in chosen if pred(recs[k], feats[k]))
        for k in sorted(range(len(recs)), key=lambda k: len(recs[k]["query"]) * len(recs[k]["target"])):
            if have >= count:
                break
            if k not in chosen and pred(recs[k], feats[k]):
                chosen.append(k)
                have += 1
    big = sum(1 for k in chosen if not cd.is_small(recs[k]))
    rest = [k for k in range(len(recs)) if k not in chosen and cd.is_small(recs[k])]
    rng.shuffle(rest)
    assert len(chosen) <= MAX_RECORDS, (role, len(chosen))
    chosen += rest[:MAX_RECORDS - len(chosen)]
    assert 4 * (len(chosen) - big) >= 3 * len(chosen), (role, big, len(chosen))
    return sorted(chosen)


def derived_sets():
    for tag, flags in (("", []), ("_alt", cd.ALT_FLAGS)):
        params = apply_flags(ex.default_params(), flags)
        cases = pool(random.Random("coding2genome derived" + tag))
        for role, spec in cd.ROLES.items():
            model = ex.Model.derived("coding2genome", *spec, params=params)
            recs = cd.refdump_derived(role, cases, ["--withsplice", "yes"] + flags)
            for r in recs:
                thin_splice(model, r)
                if "path_score" in r:                               # the builder's table replays the reference's ids
                    score, dq, dt, _ = cg.replay(model, r)
                    assert (score, dq, dt) == (r["path_score"], r["region"][2], r["region"][3]), (role, r["id"])
            feats = [cd.features(model, r) for r in recs]
            keep = select(recs, feats, role, random.Random("select" + tag + role))
            recs = [recs[k] for k in keep]
            cd.check_set(model, recs, role)
            name = "derived_coding2genome%s_%s" % (tag, role)
            write(name, recs)


def span_pool(rng, phase):
    """Tiny rectangles (2 or 3 codons against one intron of 30 or 31 bases) and a few of 8 codons: a src DP sets END in nearly
    every cell right of the first 5' site, about 14 bytes a cell in the record."""
    out = []
    for k in range(40):
        n_aa = rng.randint(2, 3)
        ci = 0 if k % 2 == 0 else rng.randint(0, n_aa - 1)            # ci = 0: the split codon's post transition within three rows
        q, t = cg.gene_pair(rng, n_aa, introns=[(ci, phase, rng.randint(30, 31))], flank_q=0 if ci == 0 else rng.choice((0, 1, 2)),
                            flank_t=0, sub=0.0, keep=2)
        out.append(("cs%d_%02d" % (phase, k), q, t))
    for k in range(4):                                              # ... and one record of eight lanes or more per set
        q, t = cg.gene_pair(rng, 8, introns=[(rng.randint(3, 5), phase, 30)], flank_q=k % 3, flank_t=0, sub=0.0, keep=2)
        out.append(("cs%d_big%d" % (phase, k), q, t))
    return out


def span_sets():
    for phase in range(3):
        dst = cd.span_dst(phase)
        recs = [r for r in cd.refdump_span(phase, span_pool(random.Random("coding2genome span %d" % phase), phase)) if cd.span_usable(r)]
        for r in recs:                                              # the dst path walks the builder's dst table
            assert cd.walk(dst, r) == (r["region"][2], r["region"][3]), r["id"]
        early = [r for r in recs if cd.span_post_row(dst, r) is not None and cd.span_post_row(dst, r) <= 3]
        lanes = [r for r in recs if cd.span_two_lanes(r)]
        keep, size = [], 0
        big = [r for r in recs if len(r["query"]) + 1 >= 8 * cd.ROWS_PER_LANE]
        for r in big[:1] + (early[:3] if phase else []) + lanes[:2] + sorted(recs, key=lambda r: len(r["end_cells"])):
            n = len(json.dumps(r, separators=(",", ":"))) + 1
            if r in keep or len(keep) >= 8 or size + n > 100000:
                continue
            keep.append(r)
            size += n
        cd.check_span_set(dst, keep, phase)
        write("span_coding2genome_phase%d" % phase, keep)


def cli_set():
    """stdout of the reference binary on cd.cli_inputs(), --model coding2genome --gappedextension no, per variant."""
    if not cd.HAVE_BINARIES:
        sys.exit("the reference binaries are not built")
    qs, ts = cd.cli_inputs()
    out = {"model": "coding2genome", "reports": ["--showvulgar", "yes", "--showalignment", "yes"] + cd.CLI_REPORTS,
           "queries": qs, "targets": ts, "variants": {}}
    with tempfile.TemporaryDirectory() as d:
        import pathlib
        for name, extra in cd.CLI_VARIANTS.items():
            ref = cd.run_pair(pathlib.Path(d), "coding2genome", cd.CLI_REPORTS + extra, {"C4GPU_BSDP_HOST": "1"}, inputs=(qs, ts))[0]
            lines = cd.stable_lines(ref)
            same = [k for k, v in out["variants"].items() if v["stdout"] == lines]
            out["variants"][name] = {"flags": extra, "stdout": same[0] if same else lines}      # (a name: that variant's lines)
    cd.check_cli(out)
    path = os.path.join(OUT, cd.CLI_SET + ".json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(cd.CLI_SET, os.path.getsize(path), "bytes,", {k: sum(l.startswith("vulgar:") for l in cd.cli_stdout(out, k)) for k in out["variants"]})


def write(name, recs):
    path = os.path.join(OUT, name + ".jsonl")
    with open(path, "w") as f:
        for r in recs:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(name, len(recs), "records,", sum(1 for r in recs if "path_score" in r), "with a path,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if not os.path.exists(REFDUMP):
        sys.exit("oracle/_ref/refdump is not built")
    derived_sets()
    span_sets()
    cli_set()
