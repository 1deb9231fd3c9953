#!/bin/bash
# Is the device code of this tree the device code of another commit?  Emits the gfx950 assembly of the library's device side for both
# (as count_valu.sh does) and compares it kernel by kernel: the set of kernel symbols, and per symbol the instruction text and the
# .amdhsa_* descriptor block.  A host-only change must leave all of it identical; the order of the kernels in the file is free.
# usage: tools/compare_device_asm.sh [commit (default HEAD)]       exit status 0: identical
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
BASE="${1:-HEAD}"
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir "$TMP/base"
git -C "$ROOT" archive "$BASE" openfhe-development_amd/csrc include | tar -x -C "$TMP/base"
emit() { hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Wno-unused-result -x hip --cuda-device-only -S "$1/openfhe-development_amd/csrc/fhe_hip.cpp" -o "$2"; }
emit "$TMP/base" "$TMP/base.s" &
emit "$ROOT" "$TMP/tree.s"
wait $!
PYTHONPATH="$ROOT/tools" python3 - "$TMP/base.s" "$TMP/tree.s" <<'PY'
import sys
from asm_kernels import kernels

base, tree = kernels(sys.argv[1]), kernels(sys.argv[2])
ntt = [k for k in base if any(n in k for n in ("ntt_static_kernel", "ntt_row8", "poly_mul_row_", "ntt_pass_kernel"))]
bad = sorted(set(base) ^ set(tree)) + sorted(k for k in set(base) & set(tree) if base[k] != tree[k])
for k in bad:
    where = "only in one of the two" if (k in base) != (k in tree) else "body differs" if base[k][0] != tree[k][0] else "descriptor differs"
    print(f"DIFFERENT {k}: {where}")
print(f"{len(base)} kernel symbols in the base ({len(ntt)} of the NTT passes), {len(tree)} in the tree, {len(bad)} different")
sys.exit(1 if bad or not base else 0)
PY
