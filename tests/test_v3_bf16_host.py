"""CR-CED's bf16 kernel (option "v3_bf16": frame16_kernel over chain::NetV3F16) as compiled for gfx950 -- no GPU needed: both
instantiations exist in the library, fit the register file without more private segment than the R-CED V2 instantiation next to
them, and hold none of the instruction sequences tools/isa_lint.py knows (the stale-accumulator pair of a 16x16x16 MFMA behind
the 16x16x32 one that wrote its srcC among them: this net's skips are added in the epilogue, not through the identity MFMA)."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin/"
SO = os.path.join(ROOT, "fullycnnspeechenhancement_amd", "librced_hip.so")


def kernel_resources(so):
    """{demangled kernel name: {vgpr, agpr, scratch}} from the amdhsa metadata notes of the embedded gfx950 code object
    (what tools/kres.py prints)."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(so))
        shutil.copy(so, local)
        subprocess.run([LLVM + "llvm-objdump", "--offloading", local], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for co in glob.glob(local + ".*gfx950*"):
            txt = subprocess.run([LLVM + "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in txt.split("- .agpr_count:")[1:]:
                blk = ".agpr_count:" + blk
                g = lambda k: re.search(r"\.%s:\s*(\S+)" % k, blk).group(1)
                name = subprocess.run(["c++filt", g("name")], check=True, capture_output=True, text=True).stdout.strip()
                out[name.split("(")[0].replace("void ", "")] = {"vgpr": int(g("vgpr_count")), "agpr": int(g("agpr_count")),
                                                                 "scratch": int(g("private_segment_fixed_size"))}
    return out


def frame16(res, net, w):
    hits = [v for k, v in res.items() if re.search(r"frame16_kernel<rced::chain::%s, %d>$" % (net, w), k)]
    assert len(hits) == 1, (net, w, sorted(res))
    return hits[0]


@pytest.mark.parametrize("w", [4, 8])
def test_cr_ced_bf16_kernel_fits_the_register_file(w, built):
    res = kernel_resources(SO)
    k3, k2 = frame16(res, "NetV3F16", w), frame16(res, "NetV2", w)
    print("\nframe16_kernel<NetV3F16, %d>: %s   <NetV2, %d>: %s" % (w, k3, w, k2))
    assert k3["vgpr"] <= 256 and k3["vgpr"] + k3["agpr"] <= 512, k3
    assert k3["scratch"] <= k2["scratch"], (k3, k2)


def test_cr_ced_bf16_kernels_are_scanned_by_the_isa_lint_and_clean(built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    assert isa_lint.default_objects() == [SO]
    with tempfile.TemporaryDirectory() as tmp:
        fns = [(fn, ins) for fn, ins in isa_lint.disassemble(SO, tmp) if "frame16_kernel" in fn and "NetV3F16" in fn]
    assert len(fns) == 2, [fn for fn, _ in fns]          # W = 4 and W = 8: what isa_lint.lint(default_objects()) walks too
    for fn, ins in fns:
        assert len(ins) > 5000, (fn, len(ins))
        mfma = [i for i in ins if i.startswith("v_mfma_")]
        # the post-ReLU skip goes through the epilogue: this net issues no identity MFMA (16x16x16) at all
        assert mfma and all(i.startswith("v_mfma_f32_16x16x32_bf16") for i in mfma), sorted({i.split()[0] for i in mfma})
        found = isa_lint.lint_function(fn, ins)
        assert not found, found[:3]
