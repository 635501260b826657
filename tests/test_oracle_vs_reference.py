"""The oracle against what the reference itself produced, recorded when the fixtures were made
(tests/golden/make_golden.py: the fixtures and tests/golden/reference_facts.json, from the imported, unmodified reference
head).  Checks (a) the committed fixtures are the ones the reference produced, on the very inputs the cases build today,
(b) the oracle agrees with them, (c) the eval skip quirk raised in the reference too (and raises in the oracle)."""
import numpy as np
import pytest

import cases
import helpers


@pytest.mark.parametrize("name", ["tiny", "ragged3", "train_tiny"] + list(cases.CLUTTERED))
def test_fixture_is_current_and_oracle_agrees(name):
    rec = helpers.load_reference_facts()["cases"][name]
    case = cases.build_case(name)
    assert helpers.content_digest(case) == rec["inputs_sha256"], "case inputs changed since the reference ran on them"
    g = helpers.load_golden(name)
    assert helpers.content_digest(g) == rec["fixture_sha256"], "fixture differs from what the reference produced"
    got = helpers.flatten_oracle(case, *helpers.run_oracle(case))
    helpers.compare_flat(got, helpers.without_gradients(g), atol=1e-6, rtol=1e-5)


def test_reference_raises_on_eval_skip_quirk():
    rec = helpers.load_reference_facts()["cases"]["skips_raise"]
    case = cases.build_case("skips_raise")
    assert helpers.content_digest(case) == rec["inputs_sha256"]
    assert rec["raises"] == "IndexError"
    with pytest.raises(IndexError):
        helpers.run_oracle(case)
