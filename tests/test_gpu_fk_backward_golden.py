"""GPU: mgr_fk_backward, mgr_fk_backward_terms and mgr_fk_backward_terms2d (csrc/fk.hip) against recorded outputs, BIT FOR BIT.
tests/golden/fk_backward_bits.npz holds the inputs of tests/fk_bits_ref.py (its docstring lists the cases) and what the three
entries gave for them on an MI355X before the two term kernels became instantiations of one template (LAB.md names the commit).
The other FK tests judge these entries against host restatements within a tolerance; this file holds their last bits in place,
so that a shared body the compiler contracts differently shows here.  Every stored case is asserted, none with a tolerance."""
import numpy as np
import pytest
import torch

import fk_bits_ref as B

pytestmark = pytest.mark.gpu
_D = B.unpack(np.load(B.GOLDEN))


def same_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_the_fixture_holds_every_case():
    names = B.case_names(_D)
    assert names == B.case_names(B.build()) and len(names) == 62
    for name in names:
        entry, dist = str(_D["case/%s/spec" % name][0]), str(_D["case/%s/spec" % name][5])
        assert "case/%s/d_theta" % name in _D
        assert ("case/%s/values" % name in _D) == (entry != "plain") and ("case/%s/dist" % name in _D) == (dist == "dist")


@pytest.mark.parametrize("name", B.case_names(_D))
def test_equals_the_recorded_bits(name):
    got = B.call(_D, name)
    want = {k: torch.tensor(_D["case/%s/%s" % (name, k)]).to(B.DEV) for k in ("d_theta", "values", "dist") if "case/%s/%s" % (name, k) in _D}
    assert sorted(got) == sorted(want)
    assert torch.equal(got["d_theta"], want["d_theta"])
    if "values" in want:
        assert want["values"].dtype == torch.float64 and torch.equal(got["values"], want["values"])
    if "dist" in want:
        assert bool(torch.isnan(want["dist"]).any()) and bool(torch.isfinite(want["dist"]).any())
        assert same_nan(got["dist"], want["dist"])
