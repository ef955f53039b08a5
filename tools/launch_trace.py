#!/usr/bin/env python
"""Every call the inference models make into the HIP library, as text: one line per call with the entry point's name, every integer
and float argument and every scalar field of a descriptor passed by reference; a pointer is 0 or 1 (null or not), the stream the
ordinal of its first appearance.  Zero-valued descriptor fields are left out.  Two commits that print the same file enqueue the same
launches with the same geometry in the same host order on the same streams.

    python tools/launch_trace.py OUT [--all OUT_ALL]
    python tools/launch_trace.py --digest OUT          # calls and SHA-256 per section of a trace written earlier

OUT holds the calls that take a stream (everything that enqueues work); OUT_ALL also the host-side size and plan queries, which are
made when buffers are allocated.  Runs 4 frames of 128x160 through the single-scene model, `LockstepScenes` (B = 2) and
`BatchedSequences` (2 scenes) in one process.  Uses only `_lib` and the public model classes, so the same file runs on any commit."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from embodied_object_detection_amd import _lib  # noqa: E402


def _value(v):
    if isinstance(v, float):
        return repr(v)
    return str(int(v))


def _fields(obj):
    """Scalar fields of a ctypes structure: pointers as 0 / 1, arrays as lists, zero fields dropped."""
    out = []
    for name, typ in obj._fields_:
        v = getattr(obj, name)
        if typ is C.c_void_p or (isinstance(typ, type) and issubclass(typ, C._Pointer)):
            v = 1 if v else 0
        elif isinstance(v, C.Array):
            v = [x for x in v]
            while v and not v[-1]:
                v.pop()
            if v:
                out.append(f"{name}=[{','.join(_value(x) for x in v)}]")
            continue
        elif isinstance(v, C.Structure):
            inner = _fields(v)
            if inner:
                out.append(f"{name}={{{inner}}}")
            continue
        if v:
            out.append(f"{name}={_value(v)}")
    return " ".join(out)


class LoggingLib:
    """Stands in for the loaded library: forwards every call, writes a line for every `eod_*` one."""

    def __init__(self, lib, launches, everything):
        self._lib, self._launches, self._everything = lib, launches, everything
        self._streams = {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("eod_"):
            return fn
        argtypes = list(fn.argtypes or [])
        takes_stream = fn.restype is C.c_int and bool(argtypes) and argtypes[-1] is C.c_void_p

        def call(*args):
            parts = [name]
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if takes_stream and i == len(argtypes) - 1:
                    parts.append(f"stream={self._streams.setdefault(a or 0, len(self._streams))}")
                elif hasattr(a, "_obj"):                               # byref(descriptor)
                    parts.append("{" + _fields(a._obj) + "}")
                elif t is C.c_void_p:
                    parts.append("1" if a else "0")
                elif isinstance(a, C.Array):
                    parts.append("[" + ",".join(_value(x) for x in a) + "]")
                elif a is None:
                    parts.append("0")
                else:
                    parts.append(_value(a))
            line = " ".join(parts) + "\n"
            if takes_stream:
                self._launches.write(line)
            if self._everything is not None:
                self._everything.write(line)
            return fn(*args)

        setattr(self, name, call)
        return call


def digest(path):
    """Per section of a trace file (`# title` lines): its number of calls and the SHA-256 over them -> text.  Two traces are the same
    file exactly when these lines are; they are what is small enough to keep beside a report."""
    import hashlib
    lines, title, n, h = [], None, 0, hashlib.sha256()
    for line in list(open(path)) + ["# end\n"]:
        if line.startswith("# "):
            if title is not None or n:
                lines.append(f"{title or 'library load'}: {n} calls, sha256 {h.hexdigest()}")
            title, n, h = line[2:].strip(), 0, hashlib.sha256()
        else:
            n += 1
            h.update(line.encode())
    return "\n".join(lines) + "\n"


def main():
    if sys.argv[1] == "--digest":           # of an existing trace file; needs no GPU
        print(digest(sys.argv[2]), end="")
        return
    out = sys.argv[1]
    out_all = sys.argv[sys.argv.index("--all") + 1] if "--all" in sys.argv else None
    launches = open(out, "w")
    everything = open(out_all, "w") if out_all else None
    # before any model is built: ops.Conv keeps the handle it gets at construction
    _lib._lib = LoggingLib(_lib.load(), launches, everything)

    import torch
    from embodied_object_detection_amd import build_model, setup_cfg
    from embodied_object_detection_amd.checkpoint import synthetic_state_dict
    from embodied_object_detection_amd.data.synthetic import SyntheticSequence
    from embodied_object_detection_amd.modeling.batched import BatchedSequences
    from embodied_object_detection_amd.modeling.lockstep import LockstepScenes

    cfg = setup_cfg(None, ["MODEL.MEMORY_TYPE", "implicit_memory", "MODEL.MAP_FEAT_FUSION", "sum", "MODEL.MAP_FEATURE_WEIGHT", 5,
                           "MODEL.DEVICE", "cuda:0"])
    sd = synthetic_state_dict(0)
    seqs = [SyntheticSequence(40 + b, H=128, W=160, n_frames=4, map_w=24, map_h=24, cell=0.5) for b in range(2)]
    eps = [[s.frame(i) for i in range(4)] for s in seqs]

    def section(title):
        for f in (launches, everything):
            if f is not None:
                f.write(f"# {title}\n")

    section("single scene: build")
    model = build_model(cfg, sd)
    section("single scene: 4 frames")
    model([eps[0]])
    torch.cuda.synchronize()
    section("LockstepScenes(B = 2): build")
    ls = LockstepScenes(cfg, 2, sd)
    section("LockstepScenes(B = 2): 4 steps")
    ls(eps)
    torch.cuda.synchronize()
    section("BatchedSequences(2): build")
    bs = BatchedSequences(cfg, 2, sd)
    section("BatchedSequences(2): 4 steps")
    bs(eps)
    torch.cuda.synchronize()
    launches.close()
    if everything is not None:
        everything.close()
    print("trace written:", out, out_all or "")
    print(digest(out), end="")


if __name__ == "__main__":
    main()
