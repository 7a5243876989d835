"""fp16 feature tables in the built library's gfx950 code objects (no GPU needed): the default path renders them on the accumulate
sweep's own fp16 form -- an instantiation of blend_accum_sweep3_kernel on the double-rate MFMA, held to the same CU-ownership
invariant as every x16 kernel -- and not on the px4 fallback."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "semantic-gaussians_amd", "sgs_hip", "libsgs_hip.so")
_spec = importlib.util.spec_from_file_location("check_code_object", os.path.join(ROOT, "semantic-gaussians_amd", "csrc", "check_code_object.py"))
cco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cco)
# blend_accum_sweep3_kernel<DBG, MM, COOP, FREE, STP, FMT>: FMT (the trailing template argument) = 1 is the fp16 form
SWEEP3 = re.compile(r"^_ZN3sgs25blend_accum_sweep3_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)ELi(\d+)EE")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(SO):
        pytest.skip("libsgs_hip.so is not built")
    if not cco.tool("llvm-objcopy") or not cco.tool("llvm-objdump"):
        pytest.skip("llvm-objcopy / llvm-objdump not found")
    pytest.importorskip("msgpack")
    return cco.scan(SO)


def _forms(kernels):
    out = {}
    for n, k in kernels.items():
        m = SWEEP3.match(n)
        if m:
            out[tuple(int(g) for g in m.groups())] = k
    return out


def test_the_default_sweep_has_an_fp16_form_on_the_double_rate_mfma(kernels):
    from sgs_hip import _lib
    forms = _forms(kernels)
    default16 = forms.get((0, 1, 0, 1, 1, 1))   # the default word 0x110004 (x16, free-running halves, store placement 1), fp16 rows
    assert default16 is not None, sorted(forms)
    assert default16["x16_instructions"] > 0
    assert default16[".vgpr_count"] == 256 and default16[".max_flat_workgroup_size"] == 512
    assert default16[".group_segment_fixed_size"] > 80 * 1024 and default16[".private_segment_fixed_size"] == 0
    assert default16["packed_f32_instructions"] == 0
    # ... and the x8 lock-step form the default falls back to when the x16 form does not own its CU
    fallback16 = forms.get((0, 0, 0, 0, 0, 1))
    assert fallback16 is not None and fallback16["x16_instructions"] == 0 and fallback16["packed_f32_instructions"] == 0
    assert fallback16[".private_segment_fixed_size"] == 0
    # the build's own reading of the code objects, with these forms in it
    assert cco.violations(kernels, _lib.load().sgs_build_flags() == 0) == []
