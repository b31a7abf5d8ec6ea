"""The bundle kernel's lane loop as compiled (tools/lane_loop_waits.py, fast
build, one compile): no flat memory instruction in it, and no wait for the
vector-memory counter between the census record's stores and the survivors'
point loop, so the stores, the n_field atomic and the next source's record
loads (pf_issue) stay in flight under the loop's VALU work."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import lane_loop_waits as LW  # noqa: E402

pytestmark = pytest.mark.skipif(LW.hipcc_path() is None, reason="hipcc not found")

KERNELS = ("c2d_bundle_kernel_fast<0,1>", "c2d_bundle_kernel_fast<0,0>")


@pytest.fixture(scope="module")
def kernels():
    return {k.name: k for k in LW.parse(LW.build_asm("fast"))}


@pytest.mark.parametrize("name", KERNELS)
def test_no_flat_in_lane_loop(kernels, name):
    k = kernels[name]
    assert k.lane_loop is not None
    loop = [i for i in k.insns if k.in_lane_loop(i)]
    # the lane loop is the bulk of the kernel, and the point loop is inside it
    assert len(loop) > len(k.insns) // 2
    assert any(i.op.startswith("v_rsq_f32") for i in loop)
    flat = ["%d: %s" % (i.line, i.text) for i in loop if i.is_flat]
    assert flat == []


@pytest.mark.parametrize("name", KERNELS)
def test_no_vmcnt_wait_from_census_stores_to_point_loop(kernels, name):
    k = kernels[name]
    rsq = next(n for n, i in enumerate(k.insns) if i.op.startswith("v_rsq_f32"))
    assert k.in_lane_loop(k.insns[rsq])
    # census_write's record: four non-temporal 16-byte stores, the last ones before the point loop
    nt = [n for n, i in enumerate(k.insns[:rsq])
          if i.op == "global_store_dwordx4" and i.text.endswith(" nt")]
    assert len(nt) >= 4
    last = nt[-1]
    between = k.insns[last + 1:rsq]
    # the prefetch of the next source's record sits in this window
    assert sum(i.op == "global_load_dwordx4" and i.text.endswith(" nt") for i in between) == 4
    waits = ["%d: %s" % (i.line, i.text) for i in between if i.is_vm_wait]
    assert waits == []
