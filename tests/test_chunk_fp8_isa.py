"""The fp8 multi-step pair kernel keeps its pointers in the global address
space (CPU test: cross-compiles rollout_loco.hip to gfx950 assembly).

The step loop of loco_pair_chunk_fp8_kernel passes every pointer through an
opaque asm once per step. A pointer that crosses it as a pointer comes back
generic, and every load of the kernel becomes flat_*: flat loads count on
vmcnt and lgkmcnt both, so the compiler drains the whole queue at every wait
and the counted waits of the set rings (vmcnt(n), n > 0) disappear. The
pointers cross as integers and are cast back to the global address space;
this test holds that in place for every instantiation, together with the
register budget the launch bounds are sized for.
"""
import importlib.util
import os
import re
import shutil

import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_ROOT, "es_pytorch_amd", "ops", "csrc", "hip", "rollout_loco.hip")
_HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
_KERNEL = "loco_pair_chunk_fp8_kernel"

pytestmark = pytest.mark.skipif(
    not (os.path.exists(_HIPCC) or shutil.which("hipcc")), reason="needs hipcc")


def _isa_loops():
    spec = importlib.util.spec_from_file_location(
        "isa_loops", os.path.join(_ROOT, "tools", "isa_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def chunk_kernels():
    """{mangled name: (body lines, resources, all lines)}, compiled once."""
    il = _isa_loops()
    if not os.path.exists(_HIPCC):
        os.environ["HIPCC"] = shutil.which("hipcc")
    lines = il.compile_asm(_SRC, [])
    names = il.kernel_names(lines, _KERNEL)
    return il, {n: (il.kernel_body(lines, n), il.resources(lines, n), lines)
                for n in names}


def test_all_instantiations_present(chunk_kernels):
    _, ks = chunk_kernels
    # <MINB, CARRY, STAGE>: MINB in {3, 4} x CARRY at STAGE 0, the staged
    # levels without carry; level 2 has the 3-block build only
    want = {"ILi3ELb0ELi0E", "ILi3ELb1ELi0E", "ILi4ELb0ELi0E", "ILi4ELb1ELi0E",
            "ILi3ELb0ELi1E", "ILi4ELb0ELi1E", "ILi3ELb0ELi2E"}
    got = {re.search(r"kernel(I\w+?E)Ev", n).group(1) for n in ks}
    assert got == want, sorted(ks)


def test_no_flat_memory_instruction(chunk_kernels):
    il, ks = chunk_kernels
    for name, (body, _, _) in ks.items():
        mem, _ = il.summary(body)
        assert sum(mem["flat"].values()) == 0, (name, dict(mem["flat"]))
        assert sum(mem["global"].values()) > 0, name


def test_counted_vmcnt_waits(chunk_kernels):
    il, ks = chunk_kernels
    for name, (body, _, _) in ks.items():
        _, waits = il.summary(body)
        counted = sum(c for form, c in waits.items()
                      for m in [re.search(r"vmcnt\((\d+)\)", form)]
                      if m and int(m.group(1)) > 0)
        assert counted >= 1, (name, dict(waits))


def test_no_scratch_no_vgpr_spill(chunk_kernels):
    il, ks = chunk_kernels
    for name, (body, res, lines) in ks.items():
        mem, _ = il.summary(body)
        assert sum(mem["scratch"].values()) == 0, (name, dict(mem["scratch"]))
        assert res["ScratchSize"] == "0", (name, res)
        # the kernel's entry in the code object metadata
        at = next(n for n, ln in enumerate(lines)
                  if re.match(r"^\s+\.name:\s+" + re.escape(name) + r"\s*$", ln))
        spill = next(int(m.group(1)) for ln in lines[at:]
                     for m in [re.match(r"^\s+\.vgpr_spill_count:\s+(\d+)", ln)] if m)
        assert spill == 0, (name, spill)
        want = 4 if "ILi4E" in name else 3
        assert int(res["Occupancy"]) == want, (name, res)
