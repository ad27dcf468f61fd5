#!/bin/bash
# ONE parameterised GPU script (replaces the per-experiment tools/gpu_r*.sh of rounds 3-4): gpurun -- 'bash tools/gpu_run.sh <section> ...'.
# Every section writes under $DN_OUT_DIR (default: out/ in the repository) and prints a short summary.  Sections:
#   df_sweep     kbench of the diffusion operator without a plan (row-GEMM back-projection); forward + backward, fp64 spot checks
#   df_modes     option "diffuse" = 0 / 2 on four batch shapes and in the block calls; workgroup start / end times of backproject_kernel
#                (libdiffnet_hip_dftrace.so = make variant TAG=dftrace EXTRA=-DDN_DF_TRACE=1)
#   df_small     df_sweep on one 7k-vertex mesh (BASELINE config 2), on 64 x 2k and on 4 x 40k meshes
#                (the one-launch kernel these three sections once swept is archived: tools/experiments/diffusion_one_launch/)
#   c256         BASELINE config 4's width: kbench block tables chained / unfused at C = 256, the C = 256 parity cases, bench.py --config cfg4
#   kbench       block_inf / block_fwd / block_bwd / diffusion tables (tools/kbench --check)
#   knn          ops.knn at the two find_knn workload shapes against chunked cdist + topk and the host KD-tree (tools/knn_timing.py)
#   knn_grid     ops.knn_grid against ops.knn in alternating windows on sphere vertices and a uniform cube, 2 000 to 1 000 000 points, the
#                grid route's steps, its counters, point_cloud_laplacian on both routes -> knn_grid_timing.txt (tools/knn_grid_timing.py)
#   fps          farthest point sampling at four shapes: the resident route, the stepped route and the torch route on the same device,
#                time per sample and launches per call -> fps_timing.txt (tools/fps_timing.py)
#   cloud        ops.knn and the point-cloud pass dn_cloud_operators_f32 at 10 000 and 200 000 points, host route at 10 000; the local-Delaunay
#                Laplacian step by step (star, emit, sort, segment sums) on the same clouds -> cloud_laplacian_timing.txt (tools/cloud_timing.py)
#   fmap         one forward + backward step of the functional map at the functional_correspondence shape: HIP route, torch route and the
#                script's row loop of torch.inverse, with launches per step (tools/fmap_timing.py)
#   geodesic     all-pairs mesh distances at the FAUST size for n_steiner = 0, 1, 3: sweeps, time of a sweep and of the device route, scipy's
#                Dijkstra scaled from 64 sources; the accuracy tables of the Steiner graph on the CPU route (tools/geodesic_timing.py)
#   eigen        the Laplacian eigenbasis at 10 000 and 2 000 vertices, k_eig = 128: the device route end to end, one product with S, the shares
#                of the dense products and of the host factorisations, eigsh on the same box -> eigenbasis_timing.txt (tools/eigen_timing.py)
#   mesh         the assembly of a mesh's operators (normals, frames, cotan Laplacian, mass, gradient operator) at 10 000 and 200 000 vertices:
#                geometry.mesh_operators on the device against the host functions on the same box, the device steps one by one
#                -> mesh_operators_timing.txt (tools/mesh_operators_timing.py)
#   tests [k]    GPU parity tier (optionally -k <expr>)
#   bench [args] bench.py (default flags: the timed steps only; add --full for the rest) -> $DN_OUT_DIR/bench.json
#   prof         rocprofv3 --kernel-trace --stats of bench.py --full -> $DN_OUT_DIR/prof/
#   suite        tests/run_gpu_suite.sh (tests group by group, smoke, bench, rocprof)
#   evidence     the round's evidence in one call: GPU tier in one process (parity margins -> JSON), default bench line, eager / chain-off /
#                three-launch-diffusion variants, rocprofv3 kernel stats + per-step kernel listing, cfg2 kernel stats, kbench tables and,
#                unless NO_PMC is set, the FETCH_SIZE / WRITE_SIZE passes and the SQ passes of the block kernels
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${DN_OUT_DIR:-$R/out}" && cd "${DN_OUT_DIR:-$R/out}" && pwd); export DN_OUT_DIR="$OUT"; cd "$R"
KB="timeout 180 ./tools/kbench"
sec=$1; shift
case "$sec" in
df_sweep)
  { echo "== three launches"; $KB --ops diffusion,diffusion_bwd --check --reps 30 --no-plan | cut -c1-170; } 2>&1 | tee $OUT/df_sweep.txt ;;
df_modes)
  { for shape in "--meshes 16 --verts 10000" "--meshes 1 --verts 7000" "--meshes 64 --verts 2000" "--meshes 1 --verts 160000"; do
      for d in 0 2; do echo "== $shape: option diffuse=$d (0 row-GEMM back-projection, 2 direct back-projection launch)"
        $KB $shape --ops diffusion,diffusion_bwd --check --reps 40 --opt diffuse=$d | grep -v "^#" | cut -c1-170; done
    done
    for d in 0 2; do echo "== blocks, 16 x 10k, diffuse=$d"; $KB --ops block_inf,block_fwd,block_bwd --reps 30 --opt diffuse=$d | grep -v "^#" | cut -c1-120; done
    for d in 0 2; do echo "== blocks, 1 x 7k, diffuse=$d"; $KB --meshes 1 --verts 7000 --ops block_inf,block_fwd,block_bwd --reps 50 --opt diffuse=$d | grep -v "^#" | cut -c1-120; done
    echo "== back-projection kernel: workgroup start / end times"; $KB --lib diffusion-net_amd/diffusion_net/libdiffnet_hip_dftrace.so --ops diffusion,diffusion_bwd --trace --reps 5 | grep -v "^#" | cut -c1-200
  } 2>&1 | tee $OUT/df_modes.txt ;;
df_small)
  { for shape in "--meshes 1 --verts 7000" "--meshes 64 --verts 2000" "--meshes 4 --verts 40000"; do
      echo "== $shape: three launches"; $KB $shape --ops diffusion,diffusion_bwd --check --reps 50 --no-plan | grep -v "^#" | cut -c1-170
    done; } 2>&1 | tee $OUT/df_small.txt ;;
c256)
  { for c in 1 0; do echo "== 1 x 200k, C = K = 256, chain=$c"; $KB --meshes 1 --verts 200000 --C 256 --K 256 --ops block_inf,block_fwd --check --reps 10 --opt chain=$c | grep -v "^#" | cut -c1-170; done
    for c in 1 0; do echo "== 16 x 10k, C = 256, K = 128, chain=$c"; $KB --C 256 --ops block_inf,block_fwd --reps 10 --opt chain=$c | grep -v "^#" | cut -c1-170; done
  } 2>&1 | tee $OUT/c256_kbench.txt
  if [ -z "$NO_TESTS" ]; then timeout 900 python -m pytest tests/test_gpu_parity.py -m gpu -q --tb=short -x -k "chained_forward_kernel_vs_unfused or chain_probes or large_inference" 2>&1 | tail -15 | tee $OUT/c256_tests.txt; fi
  timeout 300 python bench.py --config cfg4 --no-cpu-baseline --no-other-configs > $OUT/c256_bench_cfg4.json 2> $OUT/c256_bench.err; cat $OUT/c256_bench_cfg4.json | cut -c1-600; tail -3 $OUT/c256_bench.err ;;
sg256)
  { for o in 2 0; do echo "== 1 x 200k, C = K = 256, spectral_grad=$o"; $KB --meshes 1 --verts 200000 --C 256 --K 256 --ops block_inf,block_fwd --check --reps 10 --opt spectral_grad=$o | grep -v "^#" | cut -c1-170; done
    for o in 2 0; do echo "== kernel stats of block_inf, spectral_grad=$o"
      (cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/prof_s && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_s -o trace -- "$R/tools/kbench" --lib "$R/diffusion-net_amd/diffusion_net/libdiffnet_hip.so" --meshes 1 --verts 200000 --C 256 --K 256 --ops block_inf --reps 10 --opt spectral_grad=$o > /tmp/prof_s.log 2>&1 < /dev/null)
      f=$(find /tmp/prof_s -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cut -c1-160 "$f" | grep -v "rocclr\|sg_grad\|sg_pack" | head -8; done
    for o in 2 1 0; do echo "== bench cfg4, spectral_grad=$o"; timeout 300 python bench.py --config cfg4 --no-cpu-baseline --no-other-configs --lib-opt spectral_grad=$o 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'])"; done
  } 2>&1 | tee $OUT/sg256.txt
  if [ -z "$NO_TESTS" ]; then timeout 900 python -m pytest tests/test_gpu_parity.py -m gpu -q --tb=short -x -k "spectral_gradient or large_inference" 2>&1 | tail -15 | tee $OUT/sg256_tests.txt; fi ;;
bw256)
  { for d in 2 0; do echo "== 1 x 200k, C = K = 256, diffuse=$d (2: ring back-projection kernel, 0: row GEMM)"; $KB --meshes 1 --verts 200000 --C 256 --K 256 --ops diffusion,block_inf --check --reps 10 --opt diffuse=$d | grep -v "^#" | cut -c1-170; done
    for shape in "--meshes 16 --verts 10000" "--meshes 3 --verts 70000"; do for d in 2 0; do echo "== $shape, C = K = 256, diffuse=$d"; $KB $shape --C 256 --K 256 --ops diffusion,block_inf --check --reps 10 --opt diffuse=$d | grep -v "^#" | cut -c1-170; done; done
    echo "== kernel stats of block_inf, 1 x 200k"
    (cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/prof_s && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_s -o trace -- "$R/tools/kbench" --lib "$R/diffusion-net_amd/diffusion_net/libdiffnet_hip.so" --meshes 1 --verts 200000 --C 256 --K 256 --ops block_inf --reps 10 > /tmp/prof_s.log 2>&1 < /dev/null)
    f=$(find /tmp/prof_s -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cut -c1-160 "$f" | grep -v "rocclr\|sg_grad\|sg_pack" | head -9
    for d in 2 0; do echo "== bench cfg4, diffuse=$d"; timeout 300 python bench.py --config cfg4 --no-cpu-baseline --no-other-configs --lib-opt diffuse=$d 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'])"; done
  } 2>&1 | tee $OUT/bw256.txt
  if [ -z "$NO_TESTS" ]; then timeout 900 python -m pytest tests/test_gpu_parity.py -m gpu -q --tb=short -x -k "backproject_wide or large_inference or ops" 2>&1 | tail -15 | tee $OUT/bw256_tests.txt; fi ;;
kbench)
  $KB --check "$@" 2>&1 | cut -c1-200 | tee $OUT/kbench.txt ;;
knn)
  timeout 300 python tools/knn_timing.py ;;
knn_grid)
  timeout 900 python tools/knn_grid_timing.py ;;
fps)
  timeout 300 python tools/fps_timing.py ;;
cloud)
  timeout 420 python tools/cloud_timing.py ;;
fmap)
  timeout 300 python tools/fmap_timing.py ;;
geodesic)
  timeout 900 python tools/geodesic_timing.py "$@" ;;
eigen)
  timeout 420 python tools/eigen_timing.py ;;
mesh)
  timeout 420 python tools/mesh_operators_timing.py ;;
tests)
  if [ -n "$1" ]; then timeout 1500 python -m pytest tests/test_gpu_parity.py -m gpu -q --tb=short -x -k "$1" 2>&1 | tail -40 | tee $OUT/tests.txt
  else timeout 2400 python -m pytest tests -m gpu -q --tb=short -x 2>&1 | tail -40 | tee $OUT/tests.txt; fi ;;
bench)
  timeout 900 python bench.py "$@" > $OUT/bench.json 2> $OUT/bench.err; tail -c 4000 $OUT/bench.json; tail -5 $OUT/bench.err ;;
prof)
  (cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o trace -- python "$R/bench.py" --full --steps 5 --warmup 2 --no-cpu-baseline --no-other-configs "$@" > "$OUT/prof_bench.json" 2> "$OUT/prof.err")
  f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cut -c1-200 "$f" | head -40 ;;
suite)
  bash tests/run_gpu_suite.sh ;;
evidence)
  rm -f "$OUT/parity_margins_cuda.json"
  DN_PARITY_MARGINS="$OUT/parity_margins_cuda.json" timeout 1500 python -m pytest tests/ -x -q -m gpu > $OUT/gpu_tests_one_process.log 2>&1 < /dev/null; tail -3 $OUT/gpu_tests_one_process.log
  timeout 900 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err < /dev/null
  timeout 200 python bench.py --full --eager --no-cpu-baseline --no-other-configs > $OUT/bench_eager.json 2>> $OUT/bench.err < /dev/null
  timeout 200 python bench.py --full --lib-opt chain=0 --no-cpu-baseline --no-other-configs > $OUT/bench_chain_off.json 2>> $OUT/bench.err < /dev/null
  timeout 200 python bench.py --full --lib-opt diffuse=0 --no-cpu-baseline --no-other-configs > $OUT/bench_diffuse_off.json 2>> $OUT/bench.err < /dev/null
  timeout 200 python bench.py --full --lib-opt spectral_grad=2 --no-cpu-baseline --no-other-configs > $OUT/bench_spectral_always.json 2>> $OUT/bench.err < /dev/null
  timeout 200 python bench.py --full --lib-opt spectral_grad=0 --no-cpu-baseline --no-other-configs > $OUT/bench_spectral_off.json 2>> $OUT/bench.err < /dev/null
  (cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/prof_b && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_b -o trace -- python "$R/bench.py" --full --steps 10 --warmup 3 --no-cpu-baseline --no-other-configs > "$OUT/prof_bench.json" 2> "$OUT/prof.err" < /dev/null)
  f=$(find /tmp/prof_b -name "*kernel_stats.csv" 2>/dev/null | head -1); [ -n "$f" ] && cp "$f" $OUT/bench_kernel_stats.csv
  f=$(find /tmp/prof_b -name "*kernel_trace.csv" 2>/dev/null | head -1); [ -n "$f" ] && python tools/step_kernels.py "$f" > $OUT/step_kernels.txt 2>&1
  (cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/prof_c2 && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_c2 -o trace -- python "$R/bench.py" --config cfg2 --steps 40 > /dev/null 2>&1 < /dev/null)
  f=$(find /tmp/prof_c2 -name "*kernel_stats.csv" 2>/dev/null | head -1); [ -n "$f" ] && cp "$f" $OUT/cfg2_kernel_stats.csv
  (cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/prof_c4 && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_c4 -o trace -- python "$R/bench.py" --config cfg4 --steps 5 --warmup 2 --no-cpu-baseline --no-other-configs > /dev/null 2>&1 < /dev/null)
  f=$(find /tmp/prof_c4 -name "*kernel_stats.csv" 2>/dev/null | head -1); [ -n "$f" ] && cp "$f" $OUT/cfg4_kernel_stats.csv
  timeout 300 ./tools/kbench --check > $OUT/kbench.txt 2>&1 < /dev/null
  { for c in 1 0; do echo "== 1 x 200k, C = K = 256, chain=$c"; timeout 120 ./tools/kbench --meshes 1 --verts 200000 --C 256 --K 256 --ops block_inf,block_fwd --check --reps 10 --opt chain=$c | grep -v "^#" | cut -c1-170; done; } > $OUT/kbench_c256.txt 2>&1 < /dev/null
  timeout 300 ./tools/kbench --opt chain=0 --opt diffuse=0 --ops diffusion,diffusion_bwd,block_inf,block_fwd,block_bwd > $OUT/kbench_unfused.txt 2>&1 < /dev/null
  if [ -z "$NO_PMC" ]; then
    ONLY_TRAFFIC=1 timeout 600 bash tools/pmc_run.sh > $OUT/pmc_traffic.log 2>&1 < /dev/null
    (cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/prof_m && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_m -o trace -- python "$R/tools/microbench.py" --reps 3 > /dev/null 2>&1 < /dev/null)
    f=$(find /tmp/prof_m -name "*kernel_stats.csv" 2>/dev/null | head -1); [ -n "$f" ] && cp "$f" $OUT/microbench_kernel_stats.csv
    [ -f $OUT/pmc_fetch.txt ] && python tools/traffic_summary.py $OUT/pmc_fetch.txt $OUT/pmc_write.txt $OUT/microbench_kernel_stats.csv $OUT/traffic.json > $OUT/traffic_summary.log 2>&1
    OPS=diffusion,diffusion_bwd,block_fwd,block_bwd,block_inf TAG=r06 timeout 600 bash tools/pmc_kbench.sh > $OUT/pmc_sq.log 2>&1 < /dev/null
  fi
  for j in bench bench_eager bench_chain_off bench_diffuse_off bench_spectral_always bench_spectral_off; do python tools/bench_brief.py < $OUT/$j.json; done
  tail -3 $OUT/bench.err; cat $OUT/traffic_summary.log 2>/dev/null | tail -8 ;;
*) echo "unknown section $sec"; exit 1 ;;
esac
