"""CPU: csrc/meshenv_step_variant.h -- the one table of the step kernels -- against an independent transcription of the
if-chains it replaced (launch_step, meshenv_step_kernel / meshenv_rollout_kernel and MeshVecEnv's two name dicts, as they
stood before the table).  A stand-alone program that includes only that header prints the selected row for every reachable
combination of the facts; it is built with the host compiler, under the address and undefined-behaviour sanitizers."""
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc")

MAIN = r"""
#include "meshenv_step_variant.h"
#include <cstdio>
int main()
{
    using namespace meshenv;
    static_assert(sizeof(kStepVariants) / sizeof(kStepVariants[0]) == kStepVariantCount, "one table row per variant");
    static_assert(select_step_variant({false, true, false, 16, true, 272, 0}) == kGroupRagged16, "usable in constant expressions");
    std::printf("%d %d %d\n", (int)kStepVariantCount, kStepGroupVariants, kStepWaveVariants);
    const int groups[] = {1, 8, 16}, caps[] = {48, 64, 80, 128}, stages[] = {0, 2, 4, 6};
    for (int multi = 0; multi < 2; multi++)
        for (int def = 0; def < 2; def++)
            for (int moved = 0; moved < 2; moved++)
                for (int group : groups)
                    for (int ragged = 0; ragged < 2; ragged++)
                        for (int cap : caps)
                            for (int stage : stages) {
                                if ((group > 1 && !def) || (ragged && group != 16)) continue;   // not reachable
                                const StepVariant v = select_step_variant({multi != 0, def != 0, moved != 0, group, ragged != 0, cap, stage});
                                std::printf("%d %d %d %d %d %d %d|%d|%d|%s\n", multi, def, moved, group, ragged, cap, stage, (int)v,
                                            kStepVariants[v].code, kStepVariants[v].name);
                            }
    return 0;
}
"""

GROUPS, CAPS, STAGES = (1, 8, 16), (48, 64, 80, 128), (0, 2, 4, 6)


def _b(x):
    return "true" if x else "false"


def _old_launch(multi, default, moved, group, ragged, cap, stage):
    """launch_step before the table: the kernel as rocprofv3 prints it (every template argument spelled out)."""
    if not multi and group > 1 and not moved:
        if ragged:
            return "meshenv::k_step_group<16, true, true, false>"
        if cap <= 64 and group == 16:
            return "meshenv::k_step_group<16, true, false, true>"
        if cap <= 64:
            return "meshenv::k_step_group<8, true, false, true>"
        if group == 16:
            return "meshenv::k_step_group<16, true, false, false>"
        return "meshenv::k_step_group<8, true, false, false>"
    # MESHENV_LAUNCH_STEP(MULTI, DEF): k_step<kMulti, kDefaultParams, kTie = false, kSmall = false, kPre = false>
    M, D = multi, default
    if moved:
        args = (M, D, True, False, False)
    elif D and not M and (stage & 2) and cap <= 64:
        args = (False, D, False, D, D)
    elif D and not M and (stage & 2):
        args = (False, D, False, False, D)
    elif D and cap <= 64:
        args = (M, D, False, D, False)
    else:
        args = (M, D, False, False, False)
    return "meshenv::k_step<" + ", ".join(_b(a) for a in args) + ">"


def _old_step_code(default, moved, group, ragged, cap, stage):
    """meshenv_step_kernel before the table."""
    if moved:
        return 3 if default else 10
    if group <= 1:
        if not default:
            return 9
        pre = default and (stage & 2)
        return (8 if pre else 6) if default and cap <= 64 else (7 if pre else 0)
    if ragged:
        return 4
    return 5 if cap <= 64 else 1


def _old_rollout_code(default, moved, cap):
    """meshenv_rollout_kernel before the table."""
    if moved:
        return 3 if default else 4
    if not default:
        return 2
    return 1 if cap <= 64 else 0


def _old_step_name(code, group):
    """MeshVecEnv.step_kernel's dict before the table."""
    return {0: "meshenv::k_step<false, true, false, false, false>", 6: "meshenv::k_step<false, true, false, true, false>",
            7: "meshenv::k_step<false, true, false, false, true>", 8: "meshenv::k_step<false, true, false, true, true>",
            1: f"meshenv::k_step_group<{group}, true, false, false>",
            3: "meshenv::k_step<false, true, true, false, false>",
            9: "meshenv::k_step<false, false, false, false, false>", 10: "meshenv::k_step<false, false, true, false, false>",
            4: "meshenv::k_step_group<16, true, true, false>",
            5: f"meshenv::k_step_group<{group}, true, false, true>"}[code]


def _old_rollout_name(code):
    """MeshVecEnv.rollout_kernel's dict before the table."""
    return {0: "meshenv::k_step<true, true, false, false, false>", 1: "meshenv::k_step<true, true, false, true, false>",
            2: "meshenv::k_step<true, false, false, false, false>", 3: "meshenv::k_step<true, true, true, false, false>",
            4: "meshenv::k_step<true, false, true, false, false>"}[code]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the step-variant table is checked with the host C++ compiler"
    d = tmp_path_factory.mktemp("step_variant")
    src, exe = str(d / "main.cpp"), str(d / "step_variant")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]   # a sanitizer report goes to stderr and fails the run
    lines = p.stdout.strip().splitlines()
    rows = {}
    for ln in lines[1:]:
        facts, v, code, name = ln.split("|")
        rows[tuple(int(x) for x in facts.split())] = (int(v), int(code), name)
    return tuple(int(x) for x in lines[0].split()), rows


def test_the_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "meshenv_step_variant.h")).read()
    assert "#include" not in text and "__global__" not in text and "__device__" not in text


def test_every_reachable_fact_selects_what_the_old_if_chains_launched_and_reported(table):
    (count, n_group, n_wave), rows = table
    assert (count, n_group, n_wave) == (17, 5, 12)
    grid = [f for f in itertools.product((0, 1), (0, 1), (0, 1), GROUPS, (0, 1), CAPS, STAGES)
            if not (f[3] > 1 and not f[1]) and not (f[4] and f[3] != 16)]
    assert sorted(rows) == sorted(grid) and len(grid) == 2 * 2 * 16 * (1 + 1 + 1 + 2)
    for f in grid:
        multi, default, moved, group, ragged, cap, stage = f
        v, code, name = rows[f]
        launched = _old_launch(*f)
        old_code = _old_rollout_code(default, moved, cap) if multi else _old_step_code(default, moved, group, ragged, cap, stage)
        old_name = _old_rollout_name(old_code) if multi else _old_step_name(old_code, group)
        assert launched == old_name, (f, launched, old_name)   # the transcription itself: the old report was true on this grid
        assert (code, name) == (old_code, launched), (f, v, code, name, old_code, launched)
        assert (v < n_group) == name.startswith("meshenv::k_step_group<"), (f, v, name)


def test_every_row_is_reached_and_no_two_rows_share_a_name(table):
    (count, _, _), rows = table
    by_row = {}
    for v, code, name in rows.values():
        assert by_row.setdefault(v, (code, name)) == (code, name)
    assert sorted(by_row) == list(range(count))
    names = [name for _, name in by_row.values()]
    assert len(set(names)) == count
    step = {name: code for v, (code, name) in by_row.items() if "k_step<true" not in name}
    assert sorted(step.values()) == [0, 1, 1, 3, 4, 5, 5, 6, 7, 8, 9, 10]   # one code per one-step kernel, G = 8 / 16 share theirs
    assert sorted(code for v, (code, name) in by_row.items() if "k_step<true" in name) == [0, 1, 2, 3, 4]


def test_forced_group_sizes_land_on_their_rows(table):
    """What MESHENV_GROUP asks for on long rings: eight rings of the longest stride (G = 8, cap > 64), or sixteen rings
    packed by their own lengths (G = 16, ragged) -- and the same handles between a front smoothing and the next reset."""
    _, rows = table
    for cap in (80, 128):
        for stage in STAGES:
            assert rows[(0, 1, 0, 8, 0, cap, stage)][1:] == (1, "meshenv::k_step_group<8, true, false, false>")
            assert rows[(0, 1, 0, 16, 1, cap, stage)][1:] == (4, "meshenv::k_step_group<16, true, true, false>")
            assert rows[(0, 1, 1, 8, 0, cap, stage)][1:] == (3, "meshenv::k_step<false, true, true, false, false>")
            assert rows[(1, 1, 0, 16, 1, cap, stage)][1:] == (0, "meshenv::k_step<true, true, false, false, false>")
    assert rows[(0, 1, 0, 16, 1, 48, 0)][1:] == (4, "meshenv::k_step_group<16, true, true, false>")   # ragged before cap <= 64
    assert rows[(0, 1, 0, 8, 0, 64, 2)][1:] == (5, "meshenv::k_step_group<8, true, false, true>")
    assert rows[(0, 1, 0, 8, 0, 80, 2)][1:] == (1, "meshenv::k_step_group<8, true, false, false>")
