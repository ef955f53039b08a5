"""In-tree build of libeod_hip.so (gfx950) with hipcc.  `python -m embodied_object_detection_amd.build`.

The library has no dependency on torch headers: it is a flat C ABI (include/eod_hip.h) loaded with ctypes.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libeod_hip.so")
SOURCES = ["conv_igemm.hip", "conv_fp32.hip", "conv_pointwise.hip", "conv_bf16x3.hip", "conv_f16.hip", "elementwise.hip", "roi_align.hip", "select.hip", "heads.hip", "memory.hip", "semmap.hip", "place.hip", "regions.hip", "inventory.hip", "memory_read.hip", "memory_backward.hip", "conv_wgrad.hip", "train_losses.hip", "describe.hip", "relations.hip", "route.hip", "clearance.hip", "sight.hip", "frontier.hip", "obstacles.hip", "rooms.hip"]
ARCH = "gfx950"


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", h) for h in ("eod_hip.h", "eod_place.h", "eod_regions.h", "eod_inventory.h", "eod_describe.h", "eod_relations.h", "eod_route.h", "eod_clearance.h", "eod_sight.h", "eod_frontier.h", "eod_obstacles.h", "eod_rooms.h")]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _usage_file(src: str) -> str:
    return os.path.join(HERE, "build", src.replace(".hip", ".usage.txt"))


def resource_usage() -> dict:
    """{kernel symbol: {'vgprs', 'scratch', 'occupancy', 'lds'}} of the last build, from the compiler's own remarks
    (`-Rpass-analysis=kernel-resource-usage`, kept per translation unit under build/).  Empty when the library was not built here."""
    import re
    out = {}
    for src in SOURCES:
        f = _usage_file(src)
        if not os.path.exists(f):
            continue
        cur = None
        for line in open(f):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
                m = re.search(pat, line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    return out


# No kernel of the library touches scratch memory.  Round 4: one more conditional load in the shared conv epilogue spilled in the
# 128-wide and bf16x3 kernels (nothing failed; 352 -> 214 frames/s in that arithmetic), and the proposal kernels of the frame's
# critical chain kept a 168-byte copy of their argument struct in scratch because they wrote to two of its fields.
def scratch_offenders(usage: dict = None) -> list:
    usage = resource_usage() if usage is None else usage
    return sorted(k for k, v in usage.items() if v.get("scratch", 0) > 0)


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not _stale():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for src in SOURCES:
        obj = os.path.join(HERE, "build", src.replace(".hip", ".o"))
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
               "-ffp-contract=on", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd, stderr=open(_usage_file(src), "w"))))
        objs.append(obj)
    failed = [s for s, p in procs if p.wait() != 0]
    for src in SOURCES:                       # the compiler's other diagnostics (warnings, errors) still reach the terminal
        skip = 0
        held = []                                     # "In file included from" lines: they belong to the diagnostic after them
        for line in open(_usage_file(src)):
            if line.startswith("In file included from"):
                held.append(line)
                continue
            trace, held = held, []
            if "kernel-resource-usage" in line:       # a remark on a kernel of a shared header comes with its include trace
                skip = 2 if "Function Name" in line else 0      # the remark that names a kernel is followed by its source line + caret
                continue
            sys.stderr.writelines(trace)
            if skip and (line.lstrip()[:1].isdigit() or line.strip().startswith("|")):
                skip -= 1
                continue
            skip = 0
            if line.strip():
                sys.stderr.write(line)
    if failed:
        raise RuntimeError(f"hipcc failed for {failed}")
    bad = scratch_offenders()
    if bad:
        raise RuntimeError("kernels that use scratch memory (register spills / an argument struct copied to private memory): " + ", ".join(bad))
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
