#!/usr/bin/env python3
"""Code-object metadata of the built library's kernels (VGPRs, spills, scratch, LDS, code bytes), filtered by substrings
of the mangled name (template arguments read ILi128ELi16E...).

    python scripts/kernel_meta.py [substring ...]          (QUEST_HIP_LIB=<path> inspects another build)
    python scripts/kernel_meta.py --same-code OTHER.so     is every kernel's machine code (name, size, sha256) the same?
    python scripts/kernel_meta.py --same-figures OTHER.so  do the kernels both libraries have keep their resources (VGPR, spills,
                                                           scratch, LDS, SGPR, code bytes)?  Kernels only one of them has are counted.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quest_amd.build import LIB, kernel_code_hashes, kernel_metadata, library_hash  # noqa: E402

if sys.argv[1:2] == ["--same-code"]:
    mine, other = os.environ.get("QUEST_HIP_LIB") or LIB, sys.argv[2]
    a, b = kernel_code_hashes(mine), kernel_code_hashes(other)
    diff = sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))
    print(f"{len(a)} kernels (src {library_hash(mine)}) vs {len(b)} (src {library_hash(other)}): "
          + ("all equal" if not diff else f"{len(diff)} differ"))
    for n in diff:
        print(f"  {n[:100]} {a.get(n, ('-', '-'))[0]} {b.get(n, ('-', '-'))[0]}")
    sys.exit(1 if diff else 0)

if sys.argv[1:2] == ["--same-figures"]:
    mine, other = os.environ.get("QUEST_HIP_LIB") or LIB, sys.argv[2]
    a, b = kernel_metadata(mine), kernel_metadata(other)
    keys = ("vgpr", "vgpr_spill", "scratch", "lds", "sgpr", "code_bytes")
    common = sorted(set(a) & set(b))
    diff = [n for n in common if any(a[n][k] != b[n][k] for k in keys)]
    print(f"{len(a)} kernels (src {library_hash(mine)}) vs {len(b)} (src {library_hash(other)}): {len(common)} in both, "
          f"{len(set(a) - set(b))} only here, {len(set(b) - set(a))} only there; figures ({', '.join(keys)}) of the common ones: "
          + ("all equal" if not diff else f"{len(diff)} differ"))
    for n in diff:
        print(f"  {n[:100]} {[a[n][k] for k in keys]} {[b[n][k] for k in keys]}")
    sys.exit(1 if diff or set(b) - set(a) else 0)

meta = kernel_metadata(os.environ.get("QUEST_HIP_LIB") or LIB)
for name in sorted(meta):
    if sys.argv[1:] and not any(p in name for p in sys.argv[1:]):
        continue
    r = meta[name]
    short = name[len("_ZN5quest"):] if name.startswith("_ZN5quest") else name
    print(f"{short[:90]:90s} vgpr {r['vgpr']:4d} spill {r['vgpr_spill']:3d} scratch {r['scratch']:4d} lds {r['lds']:6d} "
          f"sgpr {r['sgpr']:4d} code {r['code_bytes']:6d}")
