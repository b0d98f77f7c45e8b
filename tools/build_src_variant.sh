#!/bin/bash
# Tuning aid: libmrisr_<name>.so = libmrisr.so with one or more csrc files recompiled with extra flags (each file keeps its
# FILE_FLAGS from build.py), for A/B runs on ONE box (box-to-box spread is +-1.5 %):
#   tools/build_src_variant.sh NAME FILE.hip [FILE.hip ...] [FLAGS ...]
#   MRISR_LIB=$PWD/mri_superresolution_amd/libmrisr_NAME.so python bench.py ...        (or tools/conv_bench.py)
# The classic forward kernel is compiled by the three units  IGEMM="conv_igemm_bf16.hip conv_igemm_f16.hip conv_igemm_f32.hip":
#   ablation switches (MRISR_DEBUG bits; results invalid by construction, timing only; -DMRISR_TUNING is read by
#   conv_fill_params too):
#     tools/build_src_variant.sh tune conv_fwd.hip $IGEMM conv_wgrad.hip -DMRISR_TUNING
#     MRISR_LIB=.../libmrisr_tune.so MRISR_DEBUG=8 python tools/conv_bench.py --kinds wgrad
#   phase stamps of the classic kernel (conv_fwd.hip holds the two debug entries that read them):
#     tools/build_src_variant.sh prof conv_fwd.hip $IGEMM -DMRISR_PHASE_TIMING -DMRISR_TUNING
#     MRISR_LIB=.../libmrisr_prof.so python tools/conv_bench.py --kinds fwd
#   ring kernel (MRISR_RING_DBG bits, timing only: 1 no DMA issue, 2 no MFMA, 4 no epilogue; -DMRISR_RING_PT=1 phase stamps):
#     tools/build_src_variant.sh nodma conv_ring.hip -DMRISR_RING_DBG=1
set -e
cd "$(dirname "$0")/.."
export name=$1; shift || true
srcs=(); while [[ "$1" == *.hip || "$1" == *.cpp ]]; do srcs+=("$1"); shift; done
[ -n "$name" ] && [ ${#srcs[@]} -gt 0 ] || { echo "usage: $0 NAME FILE.hip [FILE.hip ...] [FLAGS ...]" >&2; exit 2; }
python -m mri_superresolution_amd.build > /dev/null
mkdir -p build/$name
# objects of build.py's SOURCES (not whatever an older build left in build/mrisr), the named ones replaced; flags per named file
objs=$(python - "${srcs[@]}" <<'PY'
import os, runpy, sys
b = runpy.run_path("mri_superresolution_amd/build.py")
obj = lambda s: os.path.splitext(s)[0] + ".o"
print(" ".join(("build/%s/" % os.environ["name"] if s in sys.argv[1:] else "build/mrisr/") + obj(s) for s in b["SOURCES"]))
for s in sys.argv[1:]:
    print(s, *b["FLAGS"], *b["FILE_FLAGS"].get(s, []))
PY
)
{ read -r link; while read -r src flags; do
    /opt/rocm/bin/hipcc $flags "$@" -c mri_superresolution_amd/csrc/$src -o build/$name/${src%.*}.o &
done; } <<< "$objs"
for job in $(jobs -p); do wait $job; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o mri_superresolution_amd/libmrisr_$name.so $link
echo built mri_superresolution_amd/libmrisr_$name.so
