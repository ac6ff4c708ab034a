#!/bin/bash
# Build a variant of the library: some translation units recompiled with extra -D flags, the rest taken from the default build.
#   bash tests/tools/variant.sh <tag> [--unit NAME]... [--all] [--tu FILE] [-DFOO=1 ...]
# -> bliss-rs_amd/libblissgpu_<tag>.so (git-ignored; travels to the GPU box; compare with tests/tools/kbench).
#   --unit NAME   recompile NAME.hip (kernels_pairwise, kernels_fft512, scheduler, ...); may be repeated
#                 (the host-feed switches: --unit scheduler --unit blissgpu --unit node)
#   --all         recompile every unit (switches in the shared headers, e.g. -DCOARSE_SHIFT=18)
#   --tu FILE     a probe translation unit in the place of kernels_chroma.hip (it includes that file, never the other way round):
#                   tests/tools/probes/stft_trace/stft_trace.hip              per-phase cycle table of the FFT-8192 kernel, printed by kbench
#                   tests/tools/probes/handpipe/kernels_chroma_handpipe.hip   the withdrawn hand-pipelined contraction
#   with none of the three: kernels_chroma
# The units, the -ffp-contract=off units and the compiler flags are read from bliss-rs_amd/csrc/Makefile: no list is kept here.
set -euo pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); C=$R/bliss-rs_amd/csrc; HIPCC=/opt/rocm/bin/hipcc
die() { echo "variant.sh: $*" >&2; exit 2; }
all_units=$(sed -n 's/^OBJS *:= *//p' "$C/Makefile" | sed 's/\.o\>//g')
nocontract=$(sed -n 's/^\(.*\): *EXTRA *:= *\$(NOCONTRACT) *$/\1/p' "$C/Makefile" | sed 's/\.o\>//g')
flags=$(sed -n 's/^FLAGS *:= *//p' "$C/Makefile" | sed 's/\$(ARCH)/gfx950/')
[ -n "$all_units" ] && [ -n "$nocontract" ] && [ -n "$flags" ] || die "cannot read OBJS / EXTRA / FLAGS from $C/Makefile"

[ $# -ge 1 ] || die "usage: variant.sh <tag> [--unit NAME]... [--all] [--tu FILE] [-D...]"
tag=$1; shift
units=""; tu=""; defs=()
while [ $# -gt 0 ]; do
  case $1 in
    --unit) case " $all_units " in *" $2 "*) units="$units $2";; *) die "no unit '$2' in OBJS ($all_units)";; esac; shift 2;;
    --all)  units=$all_units; shift;;
    --tu)   tu=$(cd "$R" && realpath "$2"); shift 2;;
    -D*) defs+=("$1"); shift;;
    *) die "unknown argument '$1'";;
  esac
done
if [ -z "$units" ] || { [ -n "$tu" ] && [[ " $units " != *" kernels_chroma "* ]]; }; then units="$units kernels_chroma"; fi

make -C "$C" -s -j16   # the objects of the units that stay as they are
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
pids=()
for u in $units; do
  src=$C/$u.hip; extra=""
  if [ "$u" = kernels_chroma ] && [ -n "$tu" ]; then src=$tu; fi
  case " $nocontract " in *" $u "*) extra=-ffp-contract=off;; esac
  $HIPCC $flags $extra -I"$C" ${defs[@]+"${defs[@]}"} -c "$src" -o "$tmp/$u.o" & pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
objs=""
for u in $all_units; do
  if [ -f "$tmp/$u.o" ]; then objs="$objs $tmp/$u.o"; else objs="$objs $C/$u.o"; fi
done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$R/bliss-rs_amd/libblissgpu_$tag.so" $objs -ldl -Wl,-rpath,/opt/rocm/lib
echo built libblissgpu_$tag.so
