#!/usr/bin/env python
"""tools/shade_static.py FILE.s: static figures of every k_shade_path instantiation in the device assembly of tu_path.hip
(hipcc <the build's flags> --cuda-device-only -S trace.jl_amd/csrc/tu_path.hip -o FILE.s):
  registers, spill counts and scratch from the kernel's metadata, and, in program order from the kernel's entry to its first global atomic (the first emit: the matte
  path lies before it), the VALU instructions, the lane moves among them (SGPR spills to and from VGPR lanes), the v_mov and the scratch accesses."""
import re
import sys

text = open(sys.argv[1]).read()
KEYS = ("kernarg_segment_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")
print(f"{'<STREAM,TAN,DIRL>':>18} {'kernarg':>7} {'sgpr':>5} {'sgpr_spill':>10} {'vgpr':>5} {'vgpr_spill':>10} {'scratch_B':>9} | entry to first emit: {'valu':>5} {'lane_moves':>10} {'v_mov':>6} {'scratch':>7}"
      f" | whole kernel: {'valu':>6} {'lane_moves':>10}")
for blk in sorted(text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")[1:], key=lambda b: re.search(r"\.name:\s+(\S+)", b).group(1)):
    name = re.search(r"\.name:\s+(\S+)", blk).group(1)
    if "k_shade_path" not in name:
        continue
    m = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in KEYS}
    body = text[text.index("\n" + name + ":"):]
    body = body[:body.index("s_endpgm")]
    ops = [l.split()[0] for l in body.splitlines() if l.startswith("\t") and l.strip() and not l.lstrip().startswith((".", ";"))]
    head = ops[:next((k for k, op in enumerate(ops) if op.startswith("global_atomic")), len(ops))]

    def count(ls, *prefix):
        return sum(op.startswith(prefix) for op in ls)

    inst = "<" + ",".join(re.findall(r"Lb([01])E", name)[:3]) + ">"
    print(f"{inst:>18} {m['kernarg_segment_size']:>7} {m['sgpr_count']:>5} {m['sgpr_spill_count']:>10} {m['vgpr_count']:>5} {m['vgpr_spill_count']:>10} {m['private_segment_fixed_size']:>9} |"
          f" {'':>20}{count(head, 'v_'):>5} {count(head, 'v_writelane', 'v_readlane'):>10} {count(head, 'v_mov'):>6} {count(head, 'scratch_'):>7} | {'':>13}{count(ops, 'v_'):>6} {count(ops, 'v_writelane', 'v_readlane'):>10}")
