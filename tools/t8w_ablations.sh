#!/bin/bash
# In-situ ablations of conv2d_t8w (docs/LAB_NOTES.md, "What conv2d_t8w is bound by"): builds of conv2d_t8.hip with parts
# of the kernel compiled out (wrong results by design; build/variants/ only, never the product library), timed by the
# launch probe inside sequential pairs.
#   tools/t8w_ablations.sh build                   compile the variants (no GPU needed)
#   tools/t8w_ablations.sh run [launches] [form]   time tree + variants, 30 launches each -> build/t8w_ablations_formN.txt
# form 0 (the default here) is the kernel the table of the notes was measured on: the run selects it with
# PDS_DEBUG_SWITCHES=1 PDS_CONV2D_T8W_BALANCED=0; form 1 ablates the balanced form the library runs by default.
set -eo pipefail   # (a variant that fails ends the run: nothing more is started on the GPU after it)
cd "$(dirname "$0")/.."
VARIANTS="nomfma:-DPDS_C2W_NOMFMA nosplit:-DPDS_C2W_NOSPLIT noepi:-DPDS_C2W_NOEPI loadsonly:-DPDS_C2W_LOADSONLY loadsfree:-DPDS_C2W_LOADSONLY+-DPDS_C2W_NOBARRIER"
if [ "$1" = build ]; then
  pids=""
  for v in $VARIANTS; do
    tools/build_variant_one.sh t8w_${v%%:*} conv2d_t8 "$(echo ${v#*:} | tr + ' ')" &
    pids="$pids $!"
  done
  for p in $pids; do wait $p; done   # (set -e: a failed build ends the script with its status)
  exit 0
fi
N=${2:-30}
FORM=${3:-0}
export PDS_DEBUG_SWITCHES=1 PDS_CONV2D_T8W_BALANCED=$FORM
mkdir -p build
OUT=build/t8w_ablations_form$FORM.txt
echo "conv2d_t8w ablations, form $FORM" > $OUT
for v in tree $VARIANTS tree; do
  if [ "$v" = tree ]; then unset PDS_HIP_LIB; else export PDS_HIP_LIB=$PWD/build/variants/libpds_t8w_${v%%:*}.so; fi
  timeout -k 10 120 python tools/t8w_in_situ.py $N | tee -a $OUT
done
