"""The reference-made SDP record sets of coding2genome (tests/golden/sdp_coding2genome*.jsonl, made by
tools/make_coding2genome_sdp_golden.py with refdump --cmd sdp from DNA word hits, advances 1/1): what each was selected to
hold, recomputed from the records, and the oracle's SDP on every record it can judge -- those whose alignments hold neither
`phase1post ... to (END)` nor `phase2post ... to (END)` (the oracle reads the query position of a split-codon calc as an amino
acid; the reference's record is the checker everywhere else, tests/test_sdp_coding2genome_sim.py)."""
import pytest

import oracle_lib
import sdp_c2g_cases as sc


def test_default_and_altparams_hold_what_they_were_selected_for():
    ids, strips, qmod, phases, two = set(), set(), set(), {0: 0, 1: 0, 2: 0}, 0
    for name in ("sdp_coding2genome", "sdp_coding2genome_altparams"):
        model, par, recs = sc.sdp_case(name)
        assert par["dropoff"] == 50 and par["use_boundary"] == 1 and par["n_spans"] == 3
        assert 0 < len(recs) <= sc.MAX_RECORDS and all(len(r["query"]) <= sc.MAX_Q for r in recs)
        for r in recs:
            if r["alignments"]:
                ids |= sc.ids_of(r)
                strips.add(min(3, sc.strips(r)))
                qmod.add(len(r["query"]) % 3)
            for a in r["alignments"]:
                ph = sc.intron_phases(model, a)
                for p in ph:
                    phases[p] += 1
                two += len(ph) >= 2
    assert ids == set(range(model.c.n_transitions)) == set(range(30))
    assert strips == {1, 2, 3} and qmod == {0, 1, 2}
    assert min(phases.values()) >= 3 and two >= 1


def test_drop_holds_pairs_with_several_alignments():
    model, par, recs = sc.sdp_case("sdp_coding2genome_drop")
    assert par["dropoff"] == 5 and par["threshold"] == 30 and par["use_boundary"] == 1
    assert 0 < len(recs) <= sc.MAX_RECORDS and all(len(r["query"]) <= sc.MAX_Q for r in recs)
    assert sum(1 for r in recs if len(r["alignments"]) >= 2) >= 10


def test_edges_put_every_listed_event_on_its_row():
    model, par, recs = sc.sdp_case("sdp_coding2genome_edges")
    assert par["dropoff"] == 50 and 0 < len(recs) <= sc.MAX_RECORDS and all(len(r["query"]) <= sc.MAX_Q for r in recs)
    shown = set()
    for r in recs:
        built = {tuple(f) for f in r["edge"]}
        assert built and built <= sc.edge_features(model, r), r["id"]         # from the operation list: the event is on the intended row
        shown |= built
    assert shown == set(sc.EDGE_FEATURES) and len(sc.EDGE_FEATURES) == 42


@pytest.mark.parametrize("name", sorted(sc.SDP_SETS))
def test_oracle_sdp_matches_reference_where_it_can_judge(name):
    model, par, recs = sc.sdp_case(name)
    n = 0
    for r in recs:
        if not (r["alignments"] and sc.oracle_judges(r)):
            continue
        ub, got = oracle_lib.sdp(model.c, model.params, r["query"].encode(), r["target"].encode(), r["hsps"], sc.ADV[0], sc.ADV[1],
                                 par["dropoff"], True, par["threshold"], 4, qid=r["id"])
        assert ub == 1
        assert [{k: a[k] for k in sc.KEYS} for a in got] == sc.expected(r), r["id"]
        n += 1
    assert n >= 10
