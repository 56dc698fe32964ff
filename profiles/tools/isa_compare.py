#!/usr/bin/env python3
"""usage: isa_compare.py A/libpymoc_hip.so B/libpymoc_hip.so
Do two builds of the library hold the same device code?  Unbundles the gfx950 code objects of
both (llvm-objdump --offloading), and compares per kernel -- the order inside a code object may
differ -- the set of kernel symbols, the disassembly (addresses and comments stripped) and the
metadata: VGPR / AGPR / SGPR counts, scratch, static LDS, kernarg size.  Exit status 1 on any
difference."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META = (".agpr_count", ".vgpr_count", ".sgpr_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size",
        ".uses_dynamic_stack")


def kernels(lib):
  out = {}
  with tempfile.TemporaryDirectory() as tmp:
    os.symlink(os.path.abspath(lib), os.path.join(tmp, "lib.so"))
    subprocess.check_call([LLVM + "/llvm-objdump", "--offloading", "lib.so"], cwd=tmp,
                          stdout=subprocess.DEVNULL)
    for co in sorted(glob.glob(os.path.join(tmp, "lib.so*gfx950*"))):
      dis = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-leading-addr",
                                     "--no-show-raw-insn", co], text=True)
      body, cur = {}, None
      for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", ln)
        if m:
          cur = m.group(1)
          body[cur] = []
        elif cur and ln.strip():
          body[cur].append(re.sub(r"\s*//.*$", "", ln).strip())
      notes = subprocess.check_output([LLVM + "/llvm-readelf", "--notes", co], text=True)
      for blk in notes.split("  - .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        meta = tuple(re.search(r"%s:\s*(\S+)" % re.escape(k), blk).group(1) for k in META)
        assert name not in out, name
        out[name] = (len(body[name]), hashlib.sha256("\n".join(body[name]).encode()).hexdigest(), meta)
  return out


def main():
  a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
  only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
  differ = sorted(k for k in a if k in b and a[k] != b[k])
  for title, names in (("only in A", only_a), ("only in B", only_b), ("differ", differ)):
    for n in names:
      print("%s: %s %s %s" % (title, n, a.get(n, "")[::2], b.get(n, "")[::2]))
  print("%d / %d kernels, %d only in A, %d only in B, %d differ in ISA or metadata"
        % (len(a), len(b), len(only_a), len(only_b), len(differ)))
  return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
  sys.exit(main())
