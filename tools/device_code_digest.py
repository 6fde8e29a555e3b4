#!/usr/bin/env python
"""sha256 of the gfx950 device code of every source in build.SOURCES. Needs no GPU.

    python tools/device_code_digest.py [CSRC_DIR]

Each source is compiled for the device only with build.FLAGS and a fixed -cuid, which makes the object a function
of the source text alone (without -cuid the symbol hashes differ from run to run). Two source trees whose listings
are equal ship the same kernels: run it on this tree and on CSRC_DIR of another checkout and diff the output.
"""
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ruart_amd import build  # noqa: E402

EXTRA = ["-w", "-cuid=ruart", "--offload-device-only", "--no-gpu-bundle-output"]


def main():
    csrc = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else build.CSRC
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # build.FLAGS puts build.CSRC on the include path; the headers must come from the tree being digested
    flags = [csrc if f == build.CSRC else f for f in build.FLAGS] + EXTRA
    with tempfile.TemporaryDirectory() as tmp:
        def digest(name):
            obj = os.path.join(tmp, name + ".o")
            subprocess.check_call([hipcc] + flags + ["-c", os.path.join(csrc, name), "-o", obj])
            with open(obj, "rb") as f:
                data = f.read()
            return "%s  %8d  %s" % (hashlib.sha256(data).hexdigest(), len(data), name)

        with ThreadPoolExecutor(max_workers=min(16, len(build.SOURCES))) as ex:
            for line in ex.map(digest, build.SOURCES):
                print(line, flush=True)


if __name__ == "__main__":
    main()
