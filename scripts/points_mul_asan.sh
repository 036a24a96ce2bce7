#!/bin/bash
# The two host loops of csrc/points_mul.hip (the bodies k_points_mul and k_fr_powers run) under AddressSanitizer and
# UndefinedBehaviorSanitizer, as a CPU build: the host half of points_mul.hip instrumented (every sanitizer option follows
# -Xarch_host: no device code is instrumented), linked with the ordinary objects of the A/B + testing build and the
# stand-alone driver scripts/points_mul_asan_driver.cpp.  No GPU, nothing loaded into Python.
#   scripts/points_mul_asan.sh [LOG]        (needs `make -C zk-apps_amd/csrc experiments` first; LOG defaults to stdout)
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CSRC=zk-apps_amd/csrc
OUT=scripts/_bin/points_mul_asan
LOG=${1:-/dev/stdout}
SAN="-O1 -g -std=c++17 -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Wno-unused-function -Wno-option-ignored"
mkdir -p "$OUT"
# the scalars of the CPU suite against the generator, another subgroup point and infinity; expected points from the oracle
python3 - "$OUT/vectors.bin" <<'EOF'
import struct, sys
sys.path[:0] = [".", "tests"]
from oracle import bls12_381 as ec
import srs_contribute_model as model
ks = model.edge_scalars(4)
with open(sys.argv[1], "wb") as f:
    for mul, enc in ((ec.g1_mul, ec.g1_to_bytes), (ec.g2_mul, ec.g2_to_bytes)):
        cases = [(pt, k) for pt in (mul(1), mul(0x5EED0BADC0DE), None) for k in ks]
        f.write(struct.pack("<Q", len(cases)))
        f.write(b"".join(enc(pt) for pt, _ in cases))
        f.write(b"".join(ec.fr_to_bytes(k) for _, k in cases))
        f.write(b"".join(enc(mul(k, pt) if pt is not None else None) for pt, k in cases))
EOF
# the device half is compiled as the library compiles it (-O3, no debug info: at -O1 -g it takes half an hour) and never runs
$HIPCC --offload-arch=gfx950 -fPIC -fno-exceptions -DZKMI_EXPERIMENTS -DZKMI_TESTING $SAN -Xarch_device -O3 -Xarch_device -g0 -c $CSRC/points_mul.hip -o "$OUT/points_mul.o"
$HIPCC $SAN -c scripts/points_mul_asan_driver.cpp -o "$OUT/driver.o"
OBJS=$(ls $CSRC/build_exp/*.o | grep -v '/points_mul\.o$')
$HIPCC --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Wno-option-ignored -o "$OUT/driver" "$OUT/points_mul.o" "$OUT/driver.o" $OBJS -pthread -ldl
ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/driver" "$OUT/vectors.bin" > "$LOG" 2>&1
