// rtg_knobs.h -- every compile-time knob of librtg_hip.so with its product default, in one place: each kernel
// TU sees the same values, and rtg_build_info() (rtg_ops.hip) reports them.  A knob here either selects a shipped
// path or builds a measurement variant (tools/build_variants.sh).  RTG_EXP_* are measurement-only, and those that
// change results (RTG_WRONG_ANSWER_KNOBS in rtg_ops.hip) make the Python binding refuse the library.  Variants
// measured and rejected are gone from the source; DESIGN.md keeps their numbers and git history their code.
#pragma once

// ---- used by rtg_solver.cuh
#ifndef RTG_SIDES_TILES
#define RTG_SIDES_TILES 2   // 64-frame tiles (two waves each) per k_solve_sides block (round 8 sweep at five waves per
                            // SIMD: 1 tile 96.4-98.6 us per lone SoA launch against 93.8-94.7 for the parent in the same
                            // session, bench.py 3.77-3.79 G frames/s against 3.71-3.84 with 2; profiles/r08/)
#endif
#ifndef RTG_SIDES_EARLY_WORDS
#define RTG_SIDES_EARLY_WORDS 1   // FULL_BODY_POS side kernel, AoS inputs: each read-out's table word loaded into LDS
                                  // when its link is emitted (global_load_lds), not in the read-out's batch
#endif
#ifndef RTG_AOS_PRELOAD_TIPS
#define RTG_AOS_PRELOAD_TIPS 1   // AoS inputs: the gripper's hand points loaded with the wrist fit's (125 VGPRs, still
                                 // 4 waves/SIMD; AoS 111.2 vs 113.5 us, SoA unchanged, profiles/r06/arms2/)
#endif
#ifndef RTG_SIDES_SOA_WAVES
#define RTG_SIDES_SOA_WAVES 5   // k_solve_sides FULL_BODY_POS, SoA inputs: min waves per SIMD asked of the compiler (1: it
                                // picks, 4 at 101 VGPRs; 5: 96 VGPRs, 16 B/lane of spills, and the 31,024-B LDS lets
                                // five blocks share a CU; round 21's one side program: 90 VGPRs, 16 B/lane).  The other instantiations (AoS, other kinds) always get 1.
                                // bench.py (steps on two streams) 3.90-3.95 vs 3.73-3.74 G frames/s with 1 and 3.70-3.75
                                // for the parent; a lone launch 92.8-94.6 vs 93.3-94.5 vs 93.0-94.4 us: 2048 blocks fill
                                // 1280 slots 1.6 times, so only overlapping launches gain (profiles/r08/ab_*.log)
#endif
#ifndef RTG_SIDES_UNIFORM_WAVE
#define RTG_SIDES_UNIFORM_WAVE 3   // k_solve_sides: the wave index (so the side and the tile) read through readfirstlane, a
                                   // bit mask: 1 FULL_BODY_POS SoA, 2 FULL_BODY_POS AoS, 4 the other kinds.  The compiler
                                   // then keeps the side in an SGPR and branches on it with scalar branches, where it had
                                   // kept it and three values derived from it in VGPRs (spilled at 96 VGPRs: 32 -> 16
                                   // B/lane).  At five waves bench.py 3.90-3.95 vs 3.80-3.87 G frames/s without, a lone SoA
                                   // launch 92.8-94.6 vs 94.3-96.3 us, AoS 104.3-105.2 vs 104.8-106.7; the other kinds
                                   // were not measured with it (profiles/r08/ab_*.log, build new_u0)
#endif
#ifndef RTG_QUAD8_MAX_B
#define RTG_QUAD8_MAX_B 2048   // 2 <= B <= this: k_fbp_quad with 8 frames per block (one block per CU up to 2048)
#endif
#ifndef RTG_QUAD_MAX_B
#define RTG_QUAD_MAX_B 4096   // 2 <= B <= this: k_fbp_quad (swept: 16.7 vs 17.2-17.7 us up to 4096, 19.8 vs 17.5 at 8192)
#endif
#ifndef RTG_LATENCY_MAX_B
#define RTG_LATENCY_MAX_B 49152   // 2 <= B <= this: k_fbp_latency5 (swept: faster up to 49152, slower at 65536)
#endif
#ifndef RTG_EXP_HOT_INPUTS
#define RTG_EXP_HOT_INPUTS 0   // measurement knob: every side-kernel tile reads the first block's rows (wrong answers)
#endif
#ifndef RTG_EXP_TIMESTAMPS
#define RTG_EXP_TIMESTAMPS 0   // measurement knob: lane 0 of each wave records the 100 MHz wall clock at each phase
#endif                         // into body_rot (as u32 pairs) -- wrong body_rot, tools/latency_phases.py / side_phases.py
#ifndef RTG_EXP_SKIP_SIGNAL
#define RTG_EXP_SKIP_SIGNAL 0   // measurement knob: block 0's first R10 hand-over is never raised, so its partner wave
#endif                          // times out (tests the RTG_DEVERR_HANDOVER_TIMEOUT report; wrong answers)
#ifndef RTG_VEL_SEG
#define RTG_VEL_SEG 10   // linear velocity tile: rows per thread run (10: 58.0 us vs 61.2 at 20 and 68.3 at 40, with RTG_VEL_W 8)
#endif
#ifndef RTG_VEL_LDS_MIN
#define RTG_VEL_LDS_MIN 0   // A/B knob: the velocity tile's LDS request raised to this many bytes (blocks per CU)
#endif
// ---- used by rtg_fk.hip
#ifndef RTG_FK_NT_OUT
#define RTG_FK_NT_OUT 1   // the lane-group kinematics' output rows stored non-temporal (whole 1 KiB wave stores;
                          // Hu FK 88 -> 80 us, mixed 112 -> 101 us, profiles/r06/fk/nt/)
#endif
#ifndef RTG_FK_F16_MAXJ
#define RTG_FK_F16_MAXJ 36   // lane-group kinematics: 16 frames per wave (4 lanes each) up to this J, else 8 (8 lanes)
#endif
// ---- used by rtg_math.cuh
#ifndef RTG_EXP_MULR_NOBRANCH
#define RTG_EXP_MULR_NOBRANCH 0   // measurement knob: mulr_k / mulr_n without their subnormal-quotient branch (wrong
                                  // answers on rare inputs)
#endif
#ifndef RTG_EXP_NO_TABLE
#define RTG_EXP_NO_TABLE 0
#endif
#ifndef RTG_TORSO_X0
#define RTG_TORSO_X0 1   // k_solve_sides FULL_BODY_POS: the torso fit of a zero pose whose torso vectors have x = 0 runs
                         // la_gesdd3's fixed path for a zero first column alone (la_gesdd3_x0); 0: the general fit
                         // (A/B knob, same values: SoA 93.2-94.5 vs 95.3-96.6 us in one session, medians 94.6 vs 95.0 in a
                         // second; 8 rounds pooled 94.3 vs 95.6 mean; profiles/r07/ab_headline*.log)
#endif
#ifndef RTG_FIT_FAST_DIV
#define RTG_FIT_FAST_DIV 1   // the Kabsch fits' SVD (la_lartg / la_lasv2 / la_las2_min / la_lapy2): quotients by one
                             // denominator share one reciprocal (fdiv_n: the compiler's IEEE f32 sequence minus its
                             // scaling, behind a range guard) and square roots of arguments that cannot be tiny skip
                             // cr_sqrt's 2^64 scaling (cr_sqrt_nt); 0: fdiv and cr_sqrt at every such site (A/B knob,
                             // same values)
#endif
#ifndef RTG_FIT_FAST_DIV_TU
#define RTG_FIT_FAST_DIV_TU RTG_FIT_FAST_DIV   // the same per translation unit: the Makefile's IEEE_DIV_TUS get 0 (rtg_ops, so
                                               // rtg_build_info reports 0 here: k_cal_joint_quat would lose a wave)
                                               // la_lasv2 has one form for both settings since round 20: free in rtg_ops
                                               // (no register, occupancy or time change, profiles/r20/leaf_math/)
#endif
#ifndef RTG_FDIV_CORRECTIONS
#define RTG_FDIV_CORRECTIONS 1   // fdiv_n_bare: residual corrections per quotient.  2 is the compiler's sequence; 1 gives
                                 // the same bits on the whole window (proved by exhaustion, rtg_math.cuh; round 18)
#endif
#if RTG_FDIV_CORRECTIONS != 1 && RTG_FDIV_CORRECTIONS != 2
#error "RTG_FDIV_CORRECTIONS: 1 or 2 (fewer gives wrong quotients)"
#endif
#ifndef RTG_DOF_NT_STORE
#define RTG_DOF_NT_STORE 1   // A/B knob (same values): the solvers' DOF rows (whole 128-B lines) as non-temporal stores
                             // (headline 101.3 vs 104.5 us SoA, 114.4 vs 117.7 AoS; profiles/r05/nt/)
#endif
#ifndef RTG_VEL_W
#define RTG_VEL_W 8   // velocity tiles: consecutive smoothed outputs per thread (8 vs 4: linear 61.2 vs 65.1 us, angular 110.5 vs 113.1)
#endif
#ifndef RTG_DOF_NWAY
#define RTG_DOF_NWAY 4   // HuForwardModel lane groups: joint rotations per N-way group (one rare-case branch each)
#endif
#ifndef RTG_UNIT_TAB_K
#define RTG_UNIT_TAB_K 16   // the near-unit normalisation table: the 2K + 1 f32 codes around 1.0f (32: no faster,
                            // profiles/r06/unit_tab/ab_k32*)
#endif
#ifndef RTG_EULER_LIBM
#define RTG_EULER_LIBM 1   // scipy_as_euler: atan2 correctly rounded and hypot as the host libm computes it (rtg_math.cuh);
                           // 0: the device library's, whose last bits differ from the host's in a third of the angles
#endif
#ifndef RTG_UPPER_UNIT_TAB
#define RTG_UPPER_UNIT_TAB 1   // k_solve_sides UPPER_BODY: the arm maps normalise through the near-1.0f table
#endif
#ifndef RTG_ROT_UNIT_TAB
#define RTG_ROT_UNIT_TAB 1   // k_solve_sides FULL_BODY_ROT: the normalisations through the near-1.0f table
#endif
#ifndef RTG_SIDES_UNIT_TAB
#define RTG_SIDES_UNIT_TAB 7   // k_solve_sides FULL_BODY_POS, SoA: near-1.0f table normalisation at (1 fits | 2 arm maps | 4 Euler split)
#endif
#ifndef RTG_SIDES_UNIT_TAB_AOS
#define RTG_SIDES_UNIT_TAB_AOS 1   // the same for AoS: the fits only (the arm maps push it to 138-141 VGPRs, 3 waves/SIMD;
                                  // without the tip preload all sites fit in 120 but measured slower, profiles/r06/unit_tab/)
#endif
#ifndef RTG_FRAME1_UNIT_TAB
#define RTG_FRAME1_UNIT_TAB 6   // k_fbp_frame1 / k_frame_server (B = 1): the near-1.0f table at (1 fits | 6 arm maps + Euler
                                // split); 6: 12.65-12.80 vs 12.88-13.10 us (profiles/r06/unit_tab/latency/)
#endif
#ifndef RTG_FK_UNIT_TAB
#define RTG_FK_UNIT_TAB 1   // lane-group FK / inverse FK / HuForwardModel compose: qmul_norm through the near-1.0f table
#endif
#ifndef RTG_DOF_UNIT_TAB
#define RTG_DOF_UNIT_TAB 1   // HuForwardModel: joint rotations normalised through the near-1.0f (n, 1/n) table
#endif
#ifndef RTG_VEL_UNIT_TAB
#define RTG_VEL_UNIT_TAB 1   // angular velocity: the quaternion product's normalisation through the near-1.0f table
#endif
#ifndef RTG_VEL_ANG_NB
#define RTG_VEL_ANG_NB 2   // angular velocity tile: raw elements per thread per load batch (1-4 measured alike, ~110 us)
#endif
#ifndef RTG_ROT_INGEST_TILE_AOS
#define RTG_ROT_INGEST_TILE_AOS 16   // k_rot_ingest (rtg_rot_ingest.hip): frames per block of 16 T threads, AoS out; a
                                     // multiple of 4 in 8 .. 64 (8 / 16 / 32 measured alike)
#endif
#ifndef RTG_ROT_INGEST_TILE_SOA
#define RTG_ROT_INGEST_TILE_SOA 16   // the same, SoA out (16 / 32 / 64: 76 / 79 / 103 us for 23 -> 21); rtg/ingest.py
                                     // ROT_TILE_AOS / ROT_TILE_SOA repeat the two
#endif
#ifndef RTG_EXP_NO_RARE
#define RTG_EXP_NO_RARE 0  // measurement knob, a bit mask: the rare-case branches of cr_sqrt (1) / cr_acos (2) /
#endif                      // cr_sincos (4) / mulr_k and mulr_n (8: the single-quotient mulr too, which is mulr_k<1>
                            // since round 20) / sqrt_clamp_rcp (16) removed (wrong answers on rare inputs)
#ifndef RTG_EXP_STUB_SVD
#define RTG_EXP_STUB_SVD 0   // measurement knob (tools/build_variants.sh): R = identity-ish, wrong answers
#endif
