"""The literal model of the consistency groups, mvpLoopMapPoints and LoopConnections (tests/loop_detect_ref.py) on the
constructed cases (tests/loop_detect_cases.py): it gives the answers each case states.  Then the C-ABI mirror of the new
structs, the exported symbols, and the plan of the new parts (tests/cpp/loop_detect_plan_test.cpp, also under ASan/UBSan)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import loop_detect_cases as LD
import loop_detect_ref as LR
from fishbirdeyevisualslam_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,c", LD.detect_cases(), ids=[n for n, _ in LD.detect_cases()])
def test_model_consistency_groups(name, c):
    g = LD.model_graph(c["K"], c["ops"])
    cg = LR.ConsistencyGroups()
    cap = c.get("cap_groups")
    for (cands, th), (enough, groups) in zip(c["calls"], c["expect"]):
        cg.th = th
        got = cg.detect(g, [k for k in cands if 0 <= k < c["K"]])   # an out-of-range candidate is no key frame
        if cap is not None:
            cg.groups = cg.groups[:cap]                              # what fits the handle's capacity
        assert got == enough
        assert [(sorted(s), n) for s, n in cg.groups] == [(sorted(s), n) for s, n in groups]


@pytest.mark.parametrize("name,c", LD.points_cases(), ids=[n for n, _ in LD.points_cases()])
def test_model_loop_map_points(name, c):
    m = LD.ref_map(c["map"])
    g = LD.model_graph(m.K, c["ops"], m.kf_order)
    assert LR.loop_map_points(g, m, c["matched"]) == c["expect"]


@pytest.mark.parametrize("name,c", LD.connections_cases(), ids=[n for n, _ in LD.connections_cases()])
def test_model_loop_connections(name, c):
    m = LD.ref_map(c["map"])
    rows, n_counter, front = LR.loop_connections(LD.model_graph(m.K, c["ops"], m.kf_order), m, c["set"])
    assert rows == c["expect"] and n_counter == c["n_counter"] and front == c["front"]
    naive, _, _ = LR.loop_connections(LD.model_graph(m.K, c["ops"], m.kf_order), m, c["set"], snapshot_before_batch=True)
    assert naive == c.get("naive", c["expect"])


def test_the_separating_case_separates():
    c = LD.lc_entry_becomes_member_before_turn()
    assert c["naive"] != c["expect"]


def test_struct_layout_matches_the_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fishbird.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(fb_loop_groups_header), offsetof(fb_loop_groups_header, overflow), sizeof(fb_loop_connections_header), '
           'offsetof(fb_loop_connections_header, overflow), sizeof(fb_loop_connections_args), offsetof(fb_loop_connections_args, d_n_set), '
           'offsetof(fb_loop_connections_args, d_front), offsetof(fb_loop_connections_args, lc_cap), '
           'offsetof(fb_loop_connections_args, d_lc_off), offsetof(fb_loop_connections_args, d_header));return 0;}\n')
    d = tempfile.mkdtemp()
    open(os.path.join(d, "s.c"), "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    H, L, A = cabi.LoopGroupsHeader, cabi.LoopConnectionsHeader, cabi.LoopConnectionsArgs
    assert got == [C.sizeof(H), H.overflow.offset, C.sizeof(L), L.overflow.offset, C.sizeof(A), A.d_n_set.offset, A.d_front.offset,
                   A.lc_cap.offset, A.d_lc_off.offset, A.d_header.offset]


def test_new_symbols_are_listed():
    for s in ("fb_covis_detect_loop_dev", "fb_covis_detect_loop", "fb_covis_loop_groups", "fb_covis_reserve_loop_groups",
              "fb_covis_loop_map_points_dev", "fb_covis_loop_map_points", "fb_covis_reserve_loop_map_points",
              "fb_covis_loop_connections_dev", "fb_covis_loop_connections", "fb_covis_reserve_loop_connections"):
        assert s in cabi.EXPORTS


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_plan_of_the_new_parts(flags):
    exe = os.path.join(tempfile.mkdtemp(), "loop_detect_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "loop_detect_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"cases=(\d+) failures=(\d+)", r.stdout)
    assert m, r.stdout
    assert r.returncode == 0 and int(m.group(2)) == 0, r.stdout
    assert int(m.group(1)) == 10 * (6 + 5 + 3), r.stdout
