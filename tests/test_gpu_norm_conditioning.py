"""-m gpu: every route that computes a mean and a variance, on inputs whose groups / rows sit far from zero compared
with their spread (tests/norm_cases.py: r = |mu| / sigma placed at 8 and 32, plus 128 for the true two-pass routes in
fp16, and a slab / rows that are exactly constant at 64), against float64 references of the same 16-bit operands.

Most routes take their statistics in one pass (E[x^2] - mu^2 from fp32 sums), which costs about r^2 2^-24 of relative
accuracy; the rest of the suite stays at r <= 3.  A changed summation order, an fp32-for-double swap in a finisher or a
folded-LayerNorm c1 built from unrounded weights shows here and nowhere else.  tests/test_norm_cases_cpu.py shows that
fp32 two-pass arithmetic passes every case (fair) and that a one-pass fp32 model fails at r = 512 (teeth).

Each case asserts: every output - the statistics tensors an epilogue writes included, against float64 sums of the output
the same launch stored - inside the route's tolerance (``launch_audit.TOL`` by key, the audit's bounds for linear outputs
and partials, ``norm_grad_reference``'s for the backward); nothing non-finite.  In a constant case the float64 answer of
the constant slab is beta (through SiLU where it is on), so the same records cover it.  Shapes are the smallest that
reach each kernel; scripts/norm_envelope.py prints the same records from r = 0 to 512 (DESIGN.md has the table).
"""
import pytest
import torch

from tests import norm_cases as NC

pytestmark = pytest.mark.gpu

CASES = NC.cases()


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


@pytest.mark.parametrize("name,dtype,r", CASES, ids=[f"{n}-{NC.name_of(d)}-r{r}" for n, d, r in CASES])
def test_route(hip, name, dtype, r):
    NC.check(NC.run(hip, name, dtype, r), f"{name} {NC.name_of(dtype)} r={r}")


def test_every_route_of_the_table_runs_in_both_types():
    """f16 and bf16 wherever an entry point exists: tf_head, ffn_block, attn2_fused and purifier_tail have fp16 forms only."""
    half_only = {n for n, rt in NC.ROUTES.items() if rt.dtypes == NC.HALF}
    assert half_only == {"tf_head.64", "tf_head.256", "attn2_fused.lnfold", "ffn_block", "purifier_tail"}
    assert {(n, d) for n, d, _ in CASES} == {(n, d) for n, rt in NC.ROUTES.items() for d in rt.dtypes}
