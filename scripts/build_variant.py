"""A second build of the library with other compile-time geometry, for A/B runs on the GPU box (CDM_LIB=<path> selects it):
python scripts/build_variant.py <tag> <file.hip>[,<file2.hip>...] -DX=1 ...   ->  carpedeam_amd/_variants/libcarpedeam_hip_<tag>.so
Only the named files are recompiled (with the extra flags; name EVERY file that includes the header the macro lives in); the other
objects are the regular build's.  <file.hip>=<path> compiles <path> - an edited copy kept outside the tree, e.g. one with a fault put
in to see which test catches it - in the place of csrc/<file.hip>."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from carpedeam_amd import build as B  # noqa: E402

tag, srcs, flags = sys.argv[1], sys.argv[2].split(","), sys.argv[3:]
B.build()
out_dir = os.path.join(B.HERE, "_variants")
os.makedirs(out_dir, exist_ok=True)
mine = []
paths = dict(s.split("=", 1) if "=" in s else (s, os.path.join(B.CSRC, s)) for s in srcs)
srcs = list(paths)
for src in srcs:
    obj = os.path.join(out_dir, "%s_%s.o" % (src, tag))
    subprocess.run([B.HIPCC] + B.HIP_FLAGS + flags + ["-I" + B.CSRC, "-c", paths[src], "-o", obj], check=True, capture_output=True)
    mine.append(obj)
objs = [os.path.join(B.OBJ, f) for f in sorted(os.listdir(B.OBJ)) if f.endswith(".o") and f[:-2] not in srcs] + mine
lib = os.path.join(out_dir, "libcarpedeam_hip_%s.so" % tag)
# the regular library's soname, whatever the file is called: a process that loaded this variant through CDM_LIB hands it to whatever
# names libcarpedeam_hip.so as a dependency (the tests' primitives harness) instead of mapping the regular build beside it
subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-soname," + os.path.basename(B.LIB), "-o", lib] + objs + ["-lgomp"], check=True, capture_output=True)
print(lib)
