# A/B helper: build kubernetes_amd/_alt/<name>/libkschedgpu.so with one kernel source compiled
# under extra defines, or from another git revision, the other objects from the main build
# (run the main build first: one object per csrc/ksg_*.hip and csrc/*.cpp of this tree);
# load it with KSG_LIB=_alt/<name>/libkschedgpu.so (abi.py).
# usage: tools/build_alt.sh <name> <plain|window|...> [REV|-] [hipcc defines...]
set -e
cd "$(dirname "$0")/.."
NAME=$1; SRC=$2; REV=$3; shift 3
C=kubernetes_amd/csrc
O=$C/_obj
D=kubernetes_amd/_alt/$NAME
mkdir -p "$D"
F=$C/ksg_$SRC.hip
if [ "$REV" != "-" ]; then
  git show "$REV:$F" > "$D/ksg_$SRC.hip"
  F="$D/ksg_$SRC.hip"
fi
X=""
[ "$SRC" = plain_large ] && X="-mllvm -amdgpu-sched-strategy=max-ilp"
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-strict-aliasing -Wall -Wno-unused-function \
  $X -I "$C" -I include "$@" -c "$F" -o "$D/ksg_$SRC.o"
objs=""
for s in "$C"/ksg_*.hip "$C"/*.cpp; do
  k=$(basename "${s%.*}")
  if [ "$k" = "ksg_$SRC" ]; then objs="$objs $D/$k.o"; else objs="$objs $O/$k.o"; fi
done
hipcc --offload-arch=gfx950 -shared -fPIC $objs -o "$D/libkschedgpu.so" -lrccl
rm -f "$D/ksg_$SRC.o" "$D/ksg_$SRC.hip"
