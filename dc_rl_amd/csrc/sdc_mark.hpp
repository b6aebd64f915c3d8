// sdc_mark.hpp -- the plan sdc_mark_envs / sdc_rewind_envs (sdc_capi.hip) hand to sdc_mark_save_kernel and sdc_mark_rewind_kernel
// (sdc_mark.hip).
//
// A MARK ROW holds what max_steps env-steps inside one episode can change in an env, and nothing else (a snapshot row, sdc_snapshot.hpp,
// holds the env's complete state: 145 920 bytes at 672-step episodes, of which a step writes ~1.5 KB).  In the row, in this order:
//   bytes    0 ..  255   the state record (SdcRec)
//          256 ..  511   the header (SdcHdr; its four re-centring stamps H_PEND as zeros)
//          512 .. 1535   the four rank windows (qwin)
//         1536 .. 1847   the caller's obs row [3][26]
//         1848 .. 1963   the caller's share_obs row [29]
//         1964 ..        K = max_steps ring slots (dwords): the slots the next K appends go to -- what hist_append_slot (sdc_physics.hpp)
//                        yields from the record's (hist_len, hist_pos): hist_len, hist_len + 1, ... while the ring is young, then
//                        hist_pos, hist_pos + 1, ... modulo hist_cap
//         1964 + 4 K ..  K queue-table entries {cum, cumT} (two dwords each: the row's variable part is only dword-aligned) from index
//                        t_rel on; entries past the table's stride (a mark near the episode's end) are zeros and are not written back
// Rows are roundup256(1964 + 12 K) bytes apart in a caller-owned device buffer [n][row_bytes].  One launch per direction, in block ranges:
//   A  one WAVEFRONT per env (four per workgroup): the 96 sixteen-byte units of record / header / windows (lanes 0 .. 63, then 0 .. 31),
//      the 107 observation dwords (two per lane), then the 3 K dwords of the variable part, four per lane and pass.  The ring position
//      and the episode step come from the record the wavefront has just loaded -- the LIVE one on a save, the one IN THE ROW on a rewind
//      (the live record has moved on) -- with v_readlane, so no lane waits for a second, dependent load of them;
//   M  (rewind, engines with mirrors) the SLOT-MAJOR mirrors qcum_t / hist_t [slot][N]: one LANE per env, the envs in index order, so a
//      wavefront's store of one mirror row is 64 consecutive dwords wherever its envs share the slot (a lock-step batch: always for
//      qcum_t; for hist_t where the ring positions agree) and 64 scattered dwords otherwise -- the same code.  SDC_MARK_MIRROR_J steps
//      per workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define SDC_MARK_BLOCK 256
#define SDC_MARK_ENVS_PER_BLOCK 4   // range A: a wavefront per env
#define SDC_MARK_WIDE_UNITS 96      // 16-byte units of record + header + rank windows
#define SDC_MARK_OBS_DWORDS 107     // obs [3][26] + share_obs [29]
#define SDC_MARK_FIXED_BYTES 1964   // = 16 * 96 + 4 * 107: where the variable part starts
#define SDC_MARK_VAR_UNROLL 4       // dwords of the variable part a lane loads before it stores
#define SDC_MARK_MIRROR_J 8         // range M: steps per workgroup

struct SdcMarkPlan {
  const int4* idx;         // [n] {env, row, -, -} (device; rewind: sorted by env), or nullptr: env k <-> row k, n == n_envs
  int n;
  int n_envs;
  int max_steps;           // K
  int hist_cap, qstride;
  unsigned char* rows;     // the caller's buffer [n][row_bytes]
  unsigned row_bytes;
  unsigned* rec;           // [N][64]
  unsigned* hdr;           // [N][64]
  unsigned* qwin;          // [N][64][4]
  unsigned* hist;          // [N][SDC_HIST_STRIDE]
  unsigned* qtab;          // [N][qstride][2]
  float* obs;              // the caller's [N][78]
  float* share_obs;        // the caller's [N][29]
  int blocks_a, blocks_m;  // the grid is A, then M
  // rewind only
  float* obs_latch;        // the closed loop's copy of the latest observations (nullptr: none)
  unsigned* qcum_t;        // range M (blocks_m 0: none): [qstride][N]
  unsigned* hist_t;        // [hist_cap][N] (nullptr: no ring mirror)
  int m_chunks;            // ceil(K / SDC_MARK_MIRROR_J)
};

hipError_t sdc_mark_launch(const SdcMarkPlan& P, bool save, hipStream_t st);
