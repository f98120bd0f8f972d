"""Where the w-only MGS step's software-pipelined pass is selected (gk_res_plan_query,
host-only): its counted waits assume that every workgroup holds exactly 89 + 39 chunks
of 256 double2 and that nothing is streamed, so only such plans may report it."""
import pytest

import gmres_amd as ga

FULL = 2 * (89 + 39) * 256  # unknowns per workgroup of a full w-only plan


@pytest.mark.parametrize("nloc,cus,share", [(4096 * 4096, 256, 1), (512 * 512, 256, 64), (1024 * 1024, 256, 16)])
def test_full_wonly_plans_are_pipelined(nloc, cus, share):
    p = ga.res_plan_query(nloc, cus=cus, share=share)
    assert p["variant"] == "w-only" and p["r2e"] == 89 and p["l2e"] == 39, p
    assert nloc == p["G"] * FULL and p["nres2"] == nloc // 2
    assert p["pipe"] == 1, p


@pytest.mark.parametrize("nloc,cus,share,hh", [
    (4096 * 4096, 256, 1, True),       # the reflection chains keep their pass
    (520 * 520, 256, 64, False),       # a streamed rest
    (4096 * 4096 - 2, 256, 1, False),  # the last workgroup one chunk short
    (4096 * 4096, 304, 1, False),      # more CUs: fewer chunks per workgroup
    (4096 * 4096 // 2, 256, 1, False), # another variant
    (64 * 64, 256, 1, False),
])
def test_other_plans_are_not(nloc, cus, share, hh):
    p = ga.res_plan_query(nloc, cus=cus, share=share, hh=hh)
    assert p["pipe"] == 0, p
