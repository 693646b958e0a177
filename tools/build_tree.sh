# Same-box A/B of whole trees: export git revision REV into _ab/<name>/ (git archive) and
# build its libkschedgpu.so there (no UBSan twin, no oracle: its bench runs with
# --no-cpu-baseline), so `cd _ab/<name> && python bench.py ...` runs that round's library
# with that round's bench.py on the box next to the current tree's.
# The sources are whatever that revision's csrc/ holds: every ksg_*.hip (ksg_plain_large.hip,
# where there is one, under the max-ILP scheduler) and every *.cpp.
# usage: tools/build_tree.sh <name> <REV>
set -e
cd "$(dirname "$0")/.."
NAME=$1; REV=$2
D=_ab/$NAME
rm -rf "$D"; mkdir -p "$D"
git archive "$REV" | tar -x -C "$D"
C=$D/kubernetes_amd/csrc
mkdir -p "$C/_obj"
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-strict-aliasing -Wall -Wno-unused-function"
pids=""; objs=""
for s in "$C"/ksg_*.hip "$C"/*.cpp; do
  o=$C/_obj/$(basename "$s").o  # (with the extension: ksg_preempt.hip and ksg_preempt.cpp are two objects)
  X=""
  case "$s" in */ksg_plain_large.hip) X="-mllvm -amdgpu-sched-strategy=max-ilp";; esac
  hipcc $F $X -c "$s" -o "$o" & pids="$pids $!"
  objs="$objs $o"
done
for p in $pids; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC $objs -o "$D/kubernetes_amd/libkschedgpu.so" -lrccl
rm -rf "$C/_obj"
# (its tests and docs are not needed on the box)
rm -rf "$D/tests" "$D/profiles" "$D"/*.md "$D"/*_r0*.json
echo "built $D/kubernetes_amd/libkschedgpu.so from $(git rev-parse --short "$REV")"
