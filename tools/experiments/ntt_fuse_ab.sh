# same-box A/B of the common NTT pass with its tile ends fused into the outer stage pairs (k_ntt_pass8, the default) against a
# build of the parent commit (LD_LIBRARY_PATH wins over h2bench's RUNPATH, H2_LIB names the library bench.py loads), builds
# alternating, three rounds, and one plain bench.py run per build; then the knob in the new library alone (H2_NTT_FUSE=0 is
# the parent's kernel, launch for launch).  Every step under its own time limit; the first failure ends the script.
# usage: bash tools/experiments/ntt_fuse_ab.sh <directory holding the parent commit's libhalo2_hip.so>
OLD=${1:?directory of the parent libhalo2_hip.so}
SIZES="ntt 24 20 ntt 25 10 ntt 22 20 ntt 20 20"
T="timeout -k 10 120"
for round in 1 2 3; do
  echo "== new    (round $round)"; $T ./tools/h2bench $SIZES || exit 1
  echo "== parent (round $round)"; LD_LIBRARY_PATH=$OLD $T ./tools/h2bench $SIZES || exit 1
done
echo "== bench.py new";    timeout -k 10 300 python3 bench.py || exit 1
echo "== bench.py parent"; H2_LIB=$OLD/libhalo2_hip.so timeout -k 10 300 python3 bench.py || exit 1
for round in 1 2 3; do
  echo "== new, H2_NTT_FUSE=0 (round $round)"; H2_NTT_FUSE=0 $T ./tools/h2bench $SIZES || exit 1
  echo "== new, H2_NTT_FUSE=1 (round $round)"; H2_NTT_FUSE=1 $T ./tools/h2bench $SIZES || exit 1
done
