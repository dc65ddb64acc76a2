# Build an A/B variant of the product library with extra -D flags (test tooling):
#   bash tests/tools/ab_build.sh <suffix> -DFOO=1 ...  -> prostate-cancer-multimodal-segmentation_amd/libpcms_hip_<suffix>.so
# (the product Makefile with its own object directory: the source list exists once)
set -e
cd "$(dirname "$0")/../../prostate-cancer-multimodal-segmentation_amd/csrc"
SUF=$1; shift
make -j8 OUT=../libpcms_hip_$SUF.so BUILD=build_$SUF EXTRA="$*"
rm -rf build_$SUF
