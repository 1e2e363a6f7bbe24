"""The boundary tests of tests/test_gpu_reduction_boundaries.py sit where they claim to: a tiny driver compiled with g++ against
csrc/nvdr_plan.hpp (the sizing rules the gradient entry points call) evaluates every claim of PLAN_CLAIMS.  If a threshold is
retuned, this test names the boundary tests that no longer run the side of the switch they were written for."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nvdiffrast_amd", "csrc")

DRIVER = r"""
#include "nvdr_plan.hpp"
#include <cstdio>
#include <cstring>
#include <cstdlib>
int main(int argc, char** argv) {
    // each argument: rule,a,b,c,d  ->  one line with the plan's value
    for (int i = 1; i < argc; i++) {
        char rule[64] = {0};
        int a = 0, b = 0, c = 0, d = 0;
        if (std::sscanf(argv[i], "%63[a-z_],%d,%d,%d,%d", rule, &a, &b, &c, &d) < 2) return 2;
        if (!std::strcmp(rule, "tex_grad_groups")) std::printf("%d\n", nvdr_plan::tex_grad_groups(a, b, c, d != 0));
        else if (!std::strcmp(rule, "interp_grad_slots")) std::printf("%d\n", nvdr_plan::interp_grad_slots(a));
        else if (!std::strcmp(rule, "fused_grad_slots")) std::printf("%d\n", nvdr_plan::fused_grad_slots(a));
        else return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    d = tmp_path_factory.mktemp("plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(claims):
        args = [",".join([rule] + [str(int(x)) for x in (list(a) + [0, 0, 0, 0])[:4]]) for rule, a in claims]
        out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.split()
        return [int(x) for x in out]
    return run


def _claims():
    import test_gpu_reduction_boundaries as B
    return B


def test_every_boundary_test_sits_on_its_claimed_side(plan):
    B = _claims()
    got = plan([(rule, args) for rule, args, _, _ in B.PLAN_CLAIMS])
    wrong = ["%s: %s%s = %d, the test was written for %d" % (test, rule, tuple(args), g, want)
             for (rule, args, want, test), g in zip(B.PLAN_CLAIMS, got) if g != want]
    assert not wrong, "boundary tests no longer on the side they claim:\n  " + "\n  ".join(wrong)


def test_every_switch_is_straddled(plan):
    """Each step of each table is run on both sides: the claimed values cover every size the rule can produce on the way from the
    largest table to none, for the parameters the boundary tests use."""
    B = _claims()
    seen = {}
    for rule, args, want, _ in B.PLAN_CLAIMS:
        seen.setdefault(rule, set()).add(want)
    assert seen["tex_grad_groups"] >= {64, 32, 16, 0}
    assert seen["interp_grad_slots"] >= {512, 256, 128, 64, 32, 0}
    assert seen["fused_grad_slots"] >= {512, 256, 32, 0}
    # the parameter sets are adjacent across each step: the switch lies between them
    assert plan([("fused_grad_slots", (a,)) for a in (4, 5, 252, 253)]) == [512, 256, 32, 0]    # the fused table's first and last step
    for rule, params in (("interp_grad_slots", B.INTERP_A),):
        vals = plan([(rule, (a,)) for a in params])
        for a, v, a2, v2 in zip(params, vals, params[1:], vals[1:]):
            if v != v2:
                assert a2 == a + 1, "%s changes between A=%d (%d) and A=%d (%d): not adjacent, the switch is not pinned" % (rule, a, v, a2, v2)
    vals = plan([("tex_grad_groups", (c, 48, 40, 0)) for c in B.TEX_C])
    for c, v, c2, v2 in zip(B.TEX_C, vals, B.TEX_C[1:], vals[1:]):
        if v != v2:
            assert c2 == c + 1, "tex_grad_groups changes between C=%d (%d) and C=%d (%d): not adjacent" % (c, v, c2, v2)
    # the key format: the last texel extent with a table and the first without (the rule's values; the height side beyond 65536
    # texels is refused for 2-D textures and only reachable by large cube maps, so only its table side is run)
    key = plan([("tex_grad_groups", (3, 32768, 2, 0)), ("tex_grad_groups", (3, 32769, 2, 0)),
                ("tex_grad_groups", (1, 1, 65536, 0)), ("tex_grad_groups", (1, 1, 65537, 0))])
    assert min(key[0::2]) > 0 and key[1::2] == [0, 0], key
    # the 32-slot interpolate table past its 20 KiB budget: A = 80 is the first attribute count that needs more
    assert plan([("interp_grad_slots", (79,)), ("interp_grad_slots", (80,))]) == [32, 32]


def test_overflow_scene_is_sized_against_the_plan(plan):
    """test_vertex_table_overflow asserts more distinct vertices per block than OVERFLOW_SLOTS[A]: that must be at least the table
    the kernels actually get at that A."""
    B = _claims()
    for A, slots in B.OVERFLOW_SLOTS.items():
        assert slots >= max(plan([("interp_grad_slots", (A,)), ("fused_grad_slots", (A,))])), A
