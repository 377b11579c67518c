"""Residency of the edge passes (CPU: the cross-compiler's per-kernel report, shared through buildsupport.device_build()).

ADOPTED: the forms without the long-row body that run at eight waves per SIMD (profiles/README.md, "Edge passes at eight waves per
SIMD", names the same forms), each with its grouped twin: occupancy 8, no scratch.  The forms WITH the long-row body are untouched
by that work: the pin must not reach them and their code is the parent's, so their occupancy and register count are the figures of
the build before it, stated here as literals."""
import pytest

import buildsupport

ADOPTED = ("k_edge_bwd_send<1, false>", "k_edge_fwd<2, true, false>")

LONG_FORMS = {                                      # name: (VGPRs, waves per SIMD) of the build before the pins
    "k_edge_fwd<1, false, true>": (77, 6), "k_edge_fwd<2, false, true>": (72, 7),
    "k_edge_fwd<1, true, true>": (86, 5), "k_edge_fwd<2, true, true>": (80, 6),
    "k_edge_bwd_send<1, true>": (102, 4), "k_edge_bwd_send<2, true>": (104, 4),
    "k_group_edge_fwd<1, false, true>": (77, 6), "k_group_edge_fwd<2, false, true>": (72, 7),
    "k_group_edge_fwd<1, true, true>": (86, 5), "k_group_edge_fwd<2, true, true>": (80, 6),
    "k_group_edge_bwd_send<1, true>": (98, 4), "k_group_edge_bwd_send<2, true>": (98, 4),
}


@pytest.fixture(scope="module")
def usage():
    return {k.replace("void ", "").split("(")[0]: v for k, v in buildsupport.device_build().demangled().items()}


def test_adopted_forms_hold_eight_waves_without_scratch(usage):
    for solo in ADOPTED:
        for name in (solo, solo.replace("k_edge_", "k_group_edge_")):
            v = usage[name]
            assert v["occ"] == 8 and v["scratch"] == 0 and v["vgpr"] <= 64, (name, v)


def test_the_pin_does_not_reach_the_long_row_forms(usage):
    every = {n for n in usage if n.startswith(("k_edge_fwd<", "k_edge_bwd_send<", "k_group_edge_fwd<", "k_group_edge_bwd_send<")) and n.endswith("true>")}
    assert every == set(LONG_FORMS), sorted(every ^ set(LONG_FORMS))
    for name, (vgpr, occ) in LONG_FORMS.items():
        assert (usage[name]["vgpr"], usage[name]["occ"]) == (vgpr, occ), (name, usage[name])
        assert usage[name]["scratch"] == 0, (name, usage[name])
