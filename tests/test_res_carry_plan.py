"""Where the pipelined pass carries the head of its ring across the all-gather
(k_mgs_wres<.., PIPE, CARRY>, GK_TUNE_RES_PIPE_CARRY; gk_res_plan_query, host-only): only
plans that run the pipelined pass report `carry`, and they report the build's
GK_RES_PIPE_CARRY chunks."""
import os
import re

import pytest

import gmres_amd as ga
from gmres_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(path, name):
    text = open(os.path.join(ROOT, path)).read()
    m = re.search(r"^#define\s+%s\s+(-?\d+)\s*$" % name, text, re.M)
    assert m, (path, name)
    return int(m.group(1))


BUILD_CARRY = _define("gmres_amd/csrc/gk_resident.hip", "GK_RES_PIPE_CARRY")


@pytest.mark.parametrize("nloc,cus,share", [(4096 * 4096, 256, 1), (512 * 512, 256, 64), (1024 * 1024, 256, 16)])
def test_full_wonly_plans_carry_the_builds_chunks(nloc, cus, share):
    p = ga.res_plan_query(nloc, cus=cus, share=share)
    assert p["variant"] == "w-only" and p["pipe"] == 1, p
    assert p["carry"] == BUILD_CARRY, p
    assert 0 <= p["carry"] <= _define("gmres_amd/csrc/gk_resident.hip", "GK_RES_PIPE_D"), p


@pytest.mark.parametrize("nloc,cus,share,hh", [
    (4096 * 4096, 256, 1, True),       # the reflection chains keep their pass
    (520 * 520, 256, 64, False),       # a streamed rest
    (4096 * 4096 - 2, 256, 1, False),  # the last workgroup one chunk short
    (4096 * 4096, 304, 1, False),      # more CUs: fewer chunks per workgroup
    (4096 * 4096 // 2, 256, 1, False), # another variant
    (64 * 64, 256, 1, False),
])
def test_plans_without_the_pipelined_pass_carry_nothing(nloc, cus, share, hh):
    p = ga.res_plan_query(nloc, cus=cus, share=share, hh=hh)
    assert p["pipe"] == 0 and p["carry"] == 0, p


def test_info_layout_and_key_agree_with_the_header():
    hdr = "include/gmres_hip.h"
    assert len(nat.RES_INFO_KEYS) == _define(hdr, "GK_RES_INFO_LEN") == 17
    assert nat.RES_INFO_KEYS[-1] == "carry"
    assert nat.GK_TUNE_RES_PIPE_CARRY == _define(hdr, "GK_TUNE_RES_PIPE_CARRY") == 32
