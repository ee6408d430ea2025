// rt_knobs.h -- every tuning knob of rt_kernels.hip's kernels and launchers, each with the
// measurement behind its default.  All of them can be set from the command line:
// make DEFS=-DRT_TRIPS_PER_CHECK=6 BUILD=build_t6 LIB=variants/t6/lib02562rt.so (WPE= and BWPE=
// are short for RT_PATH_WAVES_PER_EU and RT_BVH_WAVES_PER_EU).  Macros only: the header
// includes nothing and can stand first anywhere.
// The diagnostic switches RT_DBG_VERT and RT_DBG_WAVE_TIMES are not knobs: they are tested
// where they are used (k_path, rt_path_kernel.h; RT_DBG_VERT also in bsp_decide,
// rt_walk_bsp.h) and have no default.
#pragma once

// ------------------------------------------------------------------ work shards
// log2 of the work shards a persistent kernel's units are dealt to (shard_of_wave,
// rt_trace_common.h): 3 = one per XCD; above 3 the low bits of the CU id within the XCD
// split each XCD's shard further.  Any value is correct, only the atomic spread changes.
// 16 or 32 shards did not pay: 32 gave config 3 +0.9 % and the BVH +1 %, but config 4 -5 %
// and config 2 -0.9 % (profiles/r02/ab_shard_count.txt)
#ifndef RT_SHARD_LG
#define RT_SHARD_LG 3
#endif
// the same for k_path's BSP instantiations alone (its BVH ones and k_trace take RT_SHARD_LG);
// 0 = one global queue, which cost config 2 39 % of its frame (profiles/r02/ab_shards.txt)
#ifndef RT_BSP_SHARDS_LG
#define RT_BSP_SHARDS_LG RT_SHARD_LG
#endif

// ------------------------------------------------------------------ BVH stack
// BVH stack split: entries [0, K) in LDS ([slot][thread], 4 B), entries [K, 50)
// in a per-lane global region ([slot - K][lane] across the grid) -- a walk
// deeper than K is rare, and the LDS share drops from 50 to K entries, which
// lets the BVH kernels run 8 waves/SIMD like the BSP ones.
#ifndef RT_BVH_LDS_ENTRIES
#define RT_BVH_LDS_ENTRIES 16
#endif

// ------------------------------------------------------------------ occupancy
// Occupancy target (waves per SIMD): the register budget the compiler fits the
// path kernel into (8 -> <= 64 VGPRs; the traversal loop keeps everything in
// registers except the hit record of an accept, and the spills sit in the
// shading code).  Measured at 256 spp: 5 waves 2744, 6: 2897, 7: 3029,
// 8: 3084 Mrays/s.
#ifndef RT_PATH_WAVES_PER_EU
#define RT_PATH_WAVES_PER_EU 8
#endif
// BVH instantiations: 8 waves/SIMD (64 VGPRs).  Round 1 measured 7 best
// (3007 Mrays/s vs 2712 at 8); with the SLP-free build and four steps per
// check 8 wins: 5792 vs 5667 (7) and 5511 (6) (profiles/r02/ab_waves2.txt)
#ifndef RT_BVH_WAVES_PER_EU
#define RT_BVH_WAVES_PER_EU 8
#endif
// W7E3 (config 2): its area-light shading keeps more state than W9E1's.  At 8
// waves/SIMD (64 VGPRs) it spilled 272 B per lane and moved 103 GB per config-2
// launch through L2 for 1 GB of sample records; at 5 (96 VGPRs) 76 B and 10 GB,
// and the frame is 3.5 % faster: 4528 vs 4375 Mrays/s (profiles/r02/ab_w7e3_waves.txt).
// With the round-2 spill cuts and per-XCD work shards, 7 waves (72 VGPRs, 52 B of
// scratch per lane) is the best: 8500 vs 7866 (5) and 8205 (8) Mrays/s
// (profiles/r02/ab_w7e3_shards.txt)
#ifndef RT_W7E3_WAVES_PER_EU
#define RT_W7E3_WAVES_PER_EU 7
#endif

// ------------------------------------------------------------------ trip loop
// traversal steps per shading-threshold check in k_path's trip loop
// (profiles/r02/ab_tpc2.txt: 2 vs 1 = config 3 +1.4%, BVH +2.6%, config 2 +0.6%;
// ab_tpc34.txt: 4 vs 2 = config 3 +1.9%, BVH +1.0%, 3 vs 2 config 2 +0.4%;
// ab_tpc8.txt: 8 vs 4 = config 3 +1.2%, config 4 +1.1%, BVH -1.2%)
#ifndef RT_TRIPS_PER_CHECK
#define RT_TRIPS_PER_CHECK 8
#endif
#ifndef RT_BVH_TRIPS_PER_CHECK
#define RT_BVH_TRIPS_PER_CHECK 4
#endif
// k_path's shading threshold is T_hi once the leaf share of the tracing lanes reaches
// NUM/DEN: 1/2 since subtree culling, which made config 4's walk 0.75 and config 5's
// 0.73 leaf tests; at 3/4 config 5 ran 2708 vs 2886 Mrays/s at 128 spp, config 4 3521
// vs 3559, configs 2 and 3 unchanged (profiles/r03/ab_ls_c*.txt)
#ifndef RT_THI_SHARE_NUM
#define RT_THI_SHARE_NUM 1
#define RT_THI_SHARE_DEN 2
#endif

// ------------------------------------------------------------------ fold
// pixel-major records k_fold loads together per thread: eight (128 B, one line).  16 and 32
// were slower: config 3's fold + unpack 1.9 ms vs 4.1 and 5.7 ms per step
// (profiles/r02/ab_fold_batch.txt)
#ifndef RT_FOLD_BATCH
#define RT_FOLD_BATCH 8
#endif
