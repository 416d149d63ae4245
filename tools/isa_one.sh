#!/bin/bash
# ISA of selected row kernels without building the whole library: direct.h's (or SRC=<unit>:
# woodbury.hip's, whiten.hip's, chol_inv.hip's, wals_big.hip's, gram_big.hip's,
# wals_heavy.hip's) kernels with explicit instantiations only.  usage:
# SRC=woodbury.hip tools/isa_one.sh out.s "template __global__ void qmfx::wals_woodbury_kernel<3, 1, false>(qmfx::SolveArgs<double>);" [compiler flags]
# SRC=whiten.hip tools/isa_one.sh out.s "template __global__ void qmfx::whiten_lds_kernel<double, 8, true>(const double*, double*, const int64_t*, int64_t, const double*, double*, double);"
# SRC=wals_big.hip tools/isa_one.sh out.s "template __global__ void qmfx::wals_big_kernel<double, 16, 0>(qmfx::SolveArgs<double>);"
set -e
OUT=$1; INST=$2; shift 2
TU=$(mktemp /tmp/isa_one_XXXX.hip)
printf '#define QMFX_KERNELS_ONLY 1\n#include "%s/qmf_amd/csrc/%s"\n%s\n' "$(cd "$(dirname "$0")/.." && pwd)" "${SRC:-direct.h}" "$INST" > $TU
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize --cuda-device-only -S "$@" $TU -o $OUT -Rpass-analysis=kernel-resource-usage 2> ${OUT%.s}.res
rm -f $TU
