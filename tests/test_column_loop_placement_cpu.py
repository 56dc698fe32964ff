"""Where the filter loops of the column twin kernel lie on the 64-byte lines of the instruction
fetch, read from the built library (no device): csrc/column.hip.h places each 16-step pass of
those loops on 8-byte addresses, because a pass that lies 4 bytes off has three lines in four
begin inside an instruction and runs 3 to 5 % slower for a lone wave.  The
placement rests on what the compiler does around one asm statement, so a compiler update or an
edit of the step can undo it without any result changing: this test is what notices.

A well placed pass has 4 to 12 of its ~550 to 730 instructions across a line, a badly placed one
41 to 57 (profiles/r08/isa_resources.md); the bound of 20 lies between the two groups."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("PYMOC_HIP_LIB") or os.path.join(ROOT, "pymoc_amd", "libpymoc_hip.so")
BOUND = 20


def _tool():
  spec = importlib.util.spec_from_file_location(
      "isa_straddle", os.path.join(ROOT, "profiles", "tools", "isa_straddle.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.mark.parametrize("kernel,count", [("k_column_steps_cls<64,2,6,true,true>", 6),
                                          ("k_column_steps_cls<64,2,2,true,true>", 2)])
def test_filter_passes_lie_on_8_byte_addresses(kernel, count):
  tool = _tool()
  if not os.path.exists(os.path.join(tool.LLVM, "llvm-objdump")):
    pytest.fail("llvm-objdump of the ROCm toolchain not found under %s" % tool.LLVM)
  # the passes of the filter loops: innermost loops of at least 400 instructions with the 16
  # v_max3_i32 of 16 steps (forms 6, 8 and 7, or the plain form; each for odd and for even nz)
  passes = [r for r in tool.rows(LIB, kernel, 400) if r[6] == 16]
  assert len(passes) == count, [(hex(r[1]), r[3]) for r in passes]
  for name, start, length, n, n8, f64, max3, cross in passes:
    assert cross <= BOUND, (name, hex(start), n, cross)
