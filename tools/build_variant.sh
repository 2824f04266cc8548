#!/bin/bash
# build_variant.sh <csrc dir> <name>: all product sources of <csrc dir> -> squeezellm_amd/ab/lib<name>.so, with the compiler, architecture,
# flags and source list of squeezellm_amd/build.py (a variant built any other way invalidates the same-box A/B it is built for)
set -e
C=$(cd "$1" && pwd); N=$2
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
mkdir -p "$R/squeezellm_amd/ab"
cd "$R"
python3 -c '
import os, subprocess, sys
from squeezellm_amd import build as B
csrc, out = sys.argv[1:3]
subprocess.run([B.hipcc(), f"--offload-arch={B.ARCH}", *B.FLAGS, "-shared", f"-I{B.INCLUDE}", f"-I{csrc}", f"-I{csrc}/experimental",
                *[os.path.join(csrc, s) for s in B.SOURCES], "-o", out], check=True)
' "$C" "$R/squeezellm_amd/ab/lib$N.so"
ls -la "$R/squeezellm_amd/ab/lib$N.so"
