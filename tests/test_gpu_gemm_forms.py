"""The GEMM launcher's switch (csrc/gemm.hip, gemm_launch; launch_f32 / launch_x3 / launch_x3d / launch_x3w): for every launchable
case of tests/gemm_forms.py — the smallest shapes at which each form of the plan is taken — ask ps_gemm_plan for the plan (it
must be the table's row), run the product through the entry the case names, and check the result against float64.  A plan row
wired to the wrong instantiation (a layout, the epilogue, the row list, the tile) computes something else; results only are
looked at.  Bound: gemm_forms.bound_of — 6e-7 of sum |a||b| + |bias| + |previous output| (tests/test_gpu_gemm_x3.py's, for
reductions of at most 1,024 terms), plus 2^-24 per split where the partial results of a longer reduction are added up."""
import pytest
import torch

import gemm_forms as gf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from prodsearch_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('name', [c['name'] for c in gf.CASES])
def test_form_matches_float64(lib, name):
    from prodsearch_amd import _lib
    case = next(c for c in gf.CASES if c['name'] == name)
    plan, err = gf.plan_of(lib, _lib, case)
    assert err is None and plan == case['plan'], (err, plan)
    outs = gf.run_case(lib, _lib, case)
    bound = gf.bound_of(case)
    for i, (got, ref, mag) in enumerate(outs):
        assert bool(torch.isfinite(got).all()), (name, i)
        e = float(((got - ref).abs() / mag).max())
        print('%s output %d: error %.3g of sum|a||b| (bound %.3g)' % (name, i, e, bound))
        assert e < bound, (name, i, e, bound)
        if case['kind'] == 'wgrad' and case['listed'][i] and case['count'] == 'empty':
            assert torch.equal(got, ref), (name, i)              # nothing listed: the output comes back bit for bit
