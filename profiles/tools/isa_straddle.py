#!/usr/bin/env python3
"""usage: isa_straddle.py libpymoc_hip.so KERNEL-SUBSTRING [MIN-INSTRUCTIONS=100]
How do the loops of a kernel lie on the 64-byte lines the instruction fetch works in?  Unbundles the
gfx950 code objects of the library (llvm-objdump --offloading), disassembles the kernels whose
demangled name (blanks removed) contains the substring, and lists every innermost loop (closed by a
backward conditional branch, no other backward branch inside): start address, length, instructions (of which
8-byte ones), fp64 arithmetic, v_max3_i32, and how many instructions lie ACROSS a 64-byte boundary.

Why it matters: the unrolled bodies of conv_spec_run are runs of 8-byte
instructions with the 4-byte ones (v_fmac_f64_e32) in close pairs, so a body either has its 8-byte
instructions on 8-byte addresses, and a handful of them cross a line, or has them 4 bytes off, and
three lines in four begin inside an instruction.  One wave per SIMD has nothing to hide that fetch
behind: the same loop measured 3 to 5 % slower in the second position."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def instructions(lib, want):
  """{kernel: [(address, bytes, opcode, operands)]} of the kernels whose name contains `want`."""
  out = {}
  with tempfile.TemporaryDirectory() as tmp:
    os.symlink(os.path.abspath(lib), os.path.join(tmp, "lib.so"))
    subprocess.check_call([LLVM + "/llvm-objdump", "--offloading", "lib.so"], cwd=tmp,
                          stdout=subprocess.DEVNULL)
    for co in sorted(glob.glob(os.path.join(tmp, "lib.so*gfx950*"))):
      # only the wanted kernels are disassembled (the whole library takes 10 s)
      syms = [ln.split()[-1] for ln in subprocess.check_output([LLVM + "/llvm-objdump", "-t", co], text=True).splitlines()
              if " F " in ln]
      names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.splitlines()
      wanted = {m: n.split("(")[0].replace("void ", "") for m, n in zip(syms, names)
                if want in n.split("(")[0].replace(" ", "")}
      if not wanted:
        continue
      dis = subprocess.check_output([LLVM + "/llvm-objdump", "-d",
                                     "--disassemble-symbols=" + ",".join(sorted(wanted)), co], text=True)
      cur = None
      for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
          cur = out.setdefault(wanted[m.group(1)], []) if m.group(1) in wanted else None
          continue
        if cur is None:
          continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*// ([0-9A-F]+): (.*)$", ln)
        if m:
          cur.append((int(m.group(3), 16), 4 * len(m.group(4).split()), m.group(1), m.group(2)))
  return out


def backward(b):
  m = re.match(r"(-?\d+)", b[3])
  return b[2].startswith("s_cbranch") and m is not None and (int(m.group(1)) >= 32768 or int(m.group(1)) < 0)


def loops(ins, least):
  index = {a: i for i, (a, _, _, _) in enumerate(ins)}
  for i, (a, size, op, args) in enumerate(ins):
    m = re.match(r"(-?\d+)", args)
    if not op.startswith("s_cbranch") or not m:
      continue
    simm = int(m.group(1))
    if simm >= 32768:
      simm -= 65536
    target = a + 4 + 4 * simm
    if target >= a or target not in index:
      continue
    body = ins[index[target]:i + 1]
    if len(body) < least or any(b[2] == "s_branch" or backward(b) for b in body[:-1]):
      continue  # (an innermost loop: forward conditional branches, the rare exits, may lie in it)
    yield target, a + size - target, body


def rows(lib, want, least=100):
  """[(kernel, start, bytes, instructions, 8-byte ones, fp64, v_max3_i32, crossings)] of every loop."""
  out = []
  for name, ins in sorted(instructions(lib, want.replace(" ", "")).items()):
    for start, length, body in loops(ins, least):
      out.append((name, start, length, len(body), sum(1 for b in body if b[1] == 8),
                  sum(1 for b in body if "_f64" in b[2] and not b[2].startswith("v_cmp")),
                  sum(1 for b in body if b[2] == "v_max3_i32"),
                  sum(1 for (x, s, _, _) in body if x // 64 != (x + s - 1) // 64)))
  return out


def main():
  least = int(sys.argv[3]) if len(sys.argv) > 3 else 100
  last = None
  for name, start, length, n, n8, f64, max3, cross in rows(sys.argv[1], sys.argv[2], least):
    if name != last:
      print("== %s" % name)
      last = name
    print("  loop at %#x (%% 64 = %2d), %5d B, %4d instructions (%4d of 8 B), fp64 %4d, v_max3_i32 %2d:"
          " %2d across a 64-byte boundary" % (start, start % 64, length, n, n8, f64, max3, cross))


if __name__ == "__main__":
  main()
