"""The training step's launch plan (csrc/train_plan.h) on the CPU: tests/train_plan_check.cpp, a stand-alone program, builds the
plan of the three nets under all 64 combinations of the six plan switches and checks that plan_train never refuses, that
every layer has one kernel of each kind, that virtual tensors and rebuilt dz are read only by kernels that rebuild them,
that every BatchNorm layer has one source of its backward sums, that every gradient tensor is stored or zeroed once and then
only added to, and that a switch leaves alone what it does not govern.  Compiled with the host compiler under
AddressSanitizer and UBSan and run as its own process; this file only compiles, runs and reports."""

import host_cxx


def test_launch_plans_of_the_three_nets_under_every_switch_combination(tmp_path):
    assert "192 plans, 0 failures" in host_cxx.run(host_cxx.build(tmp_path, "train_plan_check"), tail=4000)
