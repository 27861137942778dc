#!/bin/bash
# SQ counters of the H = 64 gradient kernel (tools/prof_grad.py: GridWorld 64x64 f32, 131072 samples per launch), three counter sets in three
# passes of their own: counters are not collected together with tracing.  Run from the repository root on the GPU box:
#   bash tools/prof_grad_pmc.sh [out.json]        (TMA_LIB_PATH selects another build of the library, PROF_OUT_DIR the output directory)
# Writes the per-launch means and the derived figures of profiles/rNN_grad_kernels_sq_pmc.json ("h64").
DIR=${PROF_OUT_DIR:-prof_out}
OUT=${1:-$DIR/grad_h64_sq_pmc.json}
mkdir -p $DIR
SQ1="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS"
SQ2="SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_VALU_MFMA_BUSY_CYCLES"
SQ3="SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_VALU_MFMA_MOPS_BF16 GRBM_GUI_ACTIVE"
i=0
for set in "$SQ1" "$SQ2" "$SQ3"; do
  i=$((i + 1))
  timeout -k 10 300 rocprofv3 --pmc $set --output-format csv -d $DIR/pmc_grad_$i -- python tools/prof_grad.py > $DIR/pmc_grad_$i.log 2>&1 || { echo "counter pass $i failed"; tail -20 $DIR/pmc_grad_$i.log; exit 1; }
done
python - "$OUT" $DIR/pmc_grad_1 $DIR/pmc_grad_2 $DIR/pmc_grad_3 <<'PY'
import collections, csv, glob, json, sys
c = {}
for d in sys.argv[2:]:
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "ppo_grad_h64" in r["Kernel_Name"]:
                per[r["Counter_Name"]][r["Dispatch_Id"]] += float(r["Counter_Value"])
    for k, v in per.items():
        c[k] = sum(v.values()) / len(v)
        print(f"  {k:32s} mean={c[k]:16.1f}  (n={len(v)})")
kc = c["SQ_BUSY_CYCLES"] / 32  # one SQ per shader engine, 32 on the chip
h = {"kernel_match": "ppo_grad_h64_kernel", "counters_mean_per_launch": c, "kernel_cycles": kc,
     "mfma_busy_cycles_per_simd": c["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024, "mfma_busy_fraction": c["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024 / kc,
     "valu_per_mfma": (c["SQ_INSTS_VALU"] - c["SQ_INSTS_MFMA"]) / c["SQ_INSTS_MFMA"],
     "active_inst_valu_quanta_cycles_per_simd": c["SQ_ACTIVE_INST_VALU"] * 4 / 1024,
     "sq_wait_any_frac_of_wave_cycles": c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"],
     "sq_wait_inst_any_frac_of_wave_cycles": c["SQ_WAIT_INST_ANY"] / c["SQ_WAVE_CYCLES"],
     "sq_active_inst_any_frac_of_wave_cycles": c["SQ_ACTIVE_INST_ANY"] / c["SQ_WAVE_CYCLES"],
     "lds_conflict_frac": c["SQ_LDS_BANK_CONFLICT"] / c["SQ_LDS_IDX_ACTIVE"]}
json.dump({"h64": h}, open(sys.argv[1], "w"), indent=1)
print({k: v for k, v in h.items() if not isinstance(v, dict)})
PY
