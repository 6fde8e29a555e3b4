#!/usr/bin/env python
"""sha256 of the gfx950 device code of every source in build.SOURCES. Needs no GPU.

    python tools/device_code_digest.py [--kernels] [CSRC_DIR]

Each source is compiled for the device only with build.FLAGS and a fixed -cuid, which makes the object a function
of the source text alone (without -cuid the symbol hashes differ from run to run). Two source trees whose listings
are equal ship the same kernels: run it on this tree and on CSRC_DIR of another checkout and diff the output.

--kernels prints one line per kernel instead of one per source: every FUNC symbol of the device object with the sha256
and the size of the bytes it spans. A change to a source then shows which of its kernels it reached.
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ruart_amd import build  # noqa: E402

EXTRA = ["-w", "-cuid=ruart", "--offload-device-only", "--no-gpu-bundle-output"]


def func_symbols(data):
    """(name, bytes) of every defined FUNC symbol of a little-endian ELF64 object, sorted by name."""
    assert data[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 object"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    # (sh_type, sh_addr, sh_offset, sh_size, sh_link, sh_entsize) per section
    sec = [struct.unpack_from("<4xI8xQQQI12xQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = []
    for typ, _, off, size, link, entsize in sec:
        if typ != 2:                                        # SHT_SYMTAB
            continue
        str_off = sec[link][2]
        for o in range(off, off + size, entsize):
            name, info, _, shndx, value, sz = struct.unpack_from("<IBBHQQ", data, o)
            if info & 0xF != 2 or shndx == 0 or shndx >= shnum:      # STT_FUNC, defined
                continue
            start = sec[shndx][2] + value - sec[shndx][1]   # (sh_addr is 0 in a relocatable object)
            end = data.index(b"\0", str_off + name)
            out.append((data[str_off + name:end].decode(), data[start:start + sz]))
    return sorted(out)


def main():
    args = [a for a in sys.argv[1:] if a != "--kernels"]
    kernels = len(args) != len(sys.argv) - 1
    csrc = os.path.abspath(args[0]) if args else build.CSRC
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # build.FLAGS puts build.CSRC on the include path; the headers must come from the tree being digested
    flags = [csrc if f == build.CSRC else f for f in build.FLAGS] + EXTRA
    with tempfile.TemporaryDirectory() as tmp:
        def digest(name):
            obj = os.path.join(tmp, name + ".o")
            subprocess.check_call([hipcc] + flags + ["-c", os.path.join(csrc, name), "-o", obj])
            with open(obj, "rb") as f:
                data = f.read()
            if kernels:
                return "\n".join("%s  %8d  %s::%s" % (hashlib.sha256(code).hexdigest(), len(code), name, sym)
                                 for sym, code in func_symbols(data))
            return "%s  %8d  %s" % (hashlib.sha256(data).hexdigest(), len(data), name)

        with ThreadPoolExecutor(max_workers=min(16, len(build.SOURCES))) as ex:
            for line in ex.map(digest, build.SOURCES):
                if line:
                    print(line, flush=True)


if __name__ == "__main__":
    main()
