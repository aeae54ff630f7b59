"""The workspace carve of the host runtime (csrc/host_carve.h, bound to a stream's buffer by csrc/host_ws.h) on the CPU:
tests/host_ws_check.cpp, a stand-alone program that never touches a device, checks that takes of float, double and int parts,
a count of 0 included, get 256-byte aligned offsets in call order, that every part is long enough and none overlaps, that
`bytes` is the end of the last part, and that rced_wave_loss_run's six parts lie where its hand-written carve put them at
(N, L, slices) = (1, 256, 1), (3, 1280, 2) and (2, 128, 1).  This file only compiles, runs and reports."""

import host_cxx


def test_carve_offsets_as_a_stand_alone_program(tmp_path):
    out = host_cxx.run(host_cxx.build(tmp_path, "host_ws_check"))
    assert " checks, 0 failures" in out and "FAILED" not in out
    assert out.count("wave loss (N ") == 18 and out.count("mixed part ") == 8
