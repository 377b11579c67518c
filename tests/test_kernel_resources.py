"""Register / LDS / scratch budgets of the kernels whose residency the launchers count on (CPU: hipcc cross-compiles gfx950 and
reports per kernel with -Rpass-analysis=kernel-resource-usage).  A couple of registers more can silently halve the number of
resident waves -- k_embed_fwd<8> went from four waves per SIMD to three that way in round 3 -- so the intended figures are pinned:
  * no kernel spills to scratch;
  * k_embed_fwd<8>: four waves per SIMD (two 8-wave blocks per CU on large row sets, launch_embed_fwd);
  * k_wgrad: two waves per SIMD (ONE resident round of two blocks per CU, place_wg);
  * k_reduce: at least six waves per SIMD and at most 26 KB of LDS (six blocks per CU: one round for ~1,200 blocks);
  * the edge passes without the long-segment body: at least six waves per SIMD."""
import pytest

import buildsupport


@pytest.fixture(scope="module")
def usage():
    return buildsupport.device_build().demangled()


def _one(usage, prefix):
    hits = [v for k, v in usage.items() if k.replace("void ", "").startswith(prefix)]
    assert len(hits) == 1, (prefix, [k for k in usage if prefix.split("<")[0] in k])
    return hits[0]


def test_no_kernel_spills(usage):
    assert len(usage) > 60
    spilled = {k: v["scratch"] for k, v in usage.items() if v.get("scratch", 0)}
    assert not spilled, spilled


def test_pinned_residency(usage):
    assert _one(usage, "k_embed_fwd<8>")["occ"] >= 4
    wg = _one(usage, "k_wgrad(")
    assert wg["occ"] == 2 and wg["vgpr"] <= 256
    rd = _one(usage, "k_reduce(")
    assert rd["occ"] >= 6 and rd["lds"] <= 26 * 1024
    for k, v in usage.items():
        name = k.replace("void ", "")
        if name.startswith("k_edge_fwd<") and name.split("(")[0].endswith("false>"):
            assert v["occ"] >= 6, (k, v)
        if name.startswith("k_edge_bwd_send<") and name.split("(")[0].endswith("false>"):
            assert v["occ"] >= 6, (k, v)
