"""The oracle's SDP (oracle/c4_oracle_sdp.c, generic in the query advance, with the 3:3 codon match) on the coding2coding model
against the reference's own alignments (tests/golden/sdp_coding2coding*.jsonl: refdump --cmd sdp from DNA word hits, advances
1/1; made by tools/make_codon_sdp_golden.py), and what those sets were selected to hold."""
import pytest

import exonerate_amd as ex
import oracle_lib
from golden_util import apply_flags, load_set

ALT_FLAGS = ["--frameshift", "-9", "--codongapopen", "-9", "--codongapextend", "-2"]
# set -> parameter flags of the model
CODON_SDP_SETS = {"sdp_coding2coding": [], "sdp_coding2coding_drop": [], "sdp_coding2coding_altparams": ALT_FLAGS}
ADV = (1, 1)
_cases = {}


def codon_sdp_case(name):
    """(model, the set's parameters, its records), loaded once."""
    if name not in _cases:
        recs = load_set(name)
        model = ex.Model("coding2coding", params=apply_flags(ex.default_params(), CODON_SDP_SETS[name]))
        _cases[name] = (model, recs[0]["params"], recs[1:])
    return _cases[name]


def expected(r):
    return [{"score": a["path_score"], "region": a["region"], "ops": a["ops"], "vulgar": a["vulgar"]} for a in r["alignments"]]


@pytest.mark.parametrize("name", sorted(CODON_SDP_SETS))
def test_oracle_sdp_matches_reference(name):
    model, par, recs = codon_sdp_case(name)
    assert par["use_boundary"] == 0 and par["singlepass"] == 1 and 0 < len(recs) <= 40
    total = 0
    for r in recs:
        ub, got = oracle_lib.sdp(model.c, model.params, r["query"].encode(), r["target"].encode(), r["hsps"], ADV[0], ADV[1],
                                 par["dropoff"], True, par["threshold"], 4, qid=r["id"])
        assert ub == 0
        got = [{k: a[k] for k in ("score", "region", "ops", "vulgar")} for a in got]
        assert got == expected(r), r["id"]
        total += len(got)
    assert total >= 10


def test_sets_hold_what_they_were_selected_for():
    ids, strips, qmod = set(), set(), set()
    for name in ("sdp_coding2coding", "sdp_coding2coding_altparams"):
        model, par, recs = codon_sdp_case(name)
        assert par["dropoff"] == 50
        for r in recs:
            if r["alignments"]:
                ids |= {t for a in r["alignments"] for t, _ in a["ops"]}
                strips.add(min(3, (len(r["query"]) + 1 + 63) // 64))
                qmod.add(len(r["query"]) % 3)
    assert ids == set(range(model.c.n_transitions)) and strips == {1, 2, 3} and qmod == {0, 1, 2}
    model, par, recs = codon_sdp_case("sdp_coding2coding_drop")
    assert par["dropoff"] == 5 and par["threshold"] == 30
    assert sum(1 for r in recs if len(r["alignments"]) >= 2) >= 10
