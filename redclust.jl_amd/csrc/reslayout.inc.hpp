// The layout of the resolver's dynamic LDS (k_resolve's tables, tab_carve) with the four constants it is sized by, host and
// device: redclust_hip.hip includes it among its first definitions, and tests/test_resolver_setup_image.py compiles it, with
// __host__ and __device__ defined away, into a small program that prints the byte counts it asserts on.  Nothing but <cstddef>.
#pragma once
#include <cstddef>

#ifndef RC_PTS
#define RC_PTS 32           // points per chunk of the resolver (a power of two <= 32): a block's threads are RC_PTS points x (threads / RC_PTS)
                            // candidate streams; chunks are dealt to the blocks cyclically.  Finer chunks would spread the points still
                            // open in a later round of a sweep — a suffix of the point order — over more blocks (at n = 8192 a 32-point
                            // chunk is all a block has), but every chunk pays the pass's fixed costs (block barriers, the reduction
                            // over the streams): measured in the moving regime 2,520 sweeps/s with 32, 2,490 with 16, 2,020 with 8
#endif
#define RC_USED_LDS_MAX_N 16384   // up to this n the label-occupancy bitset of the resolver lives in LDS (n/8 bytes)
#define RC_MAXB 512          // tentative changers validated per resolve round
#define RC_CPB_LDS 4         // chunks per block up to which k_resolve keeps its points' indices and slots in LDS (Tab::cu / cown)

#define RC_A16(x) (((x) + 15) & ~(size_t)15)
#define RC_TAB_NOFF 30
__host__ __device__ inline size_t tab_layout(int kcap, int n, int nw, size_t *off /*RC_TAB_NOFF*/, int maxb = RC_MAXB)
{
    size_t o = 0;
    off[0] = o; o = RC_A16(o + sizeof(double) * kcap);          // base_o
    off[1] = o; o = RC_A16(o + sizeof(double) * kcap);          // base_s
    off[2] = o; o = RC_A16(o + sizeof(double) * nw * RC_PTS);   // red_v
    off[3] = o; o = RC_A16(o + sizeof(unsigned long long));     // blk_key
    off[4] = o; o = RC_A16(o + sizeof(int) * kcap);             // size
    off[5] = o; o = RC_A16(o + sizeof(int) * kcap);             // label
    off[6] = o; o = RC_A16(o + sizeof(int) * nw * RC_PTS);      // red_pos
    off[7] = o; o = RC_A16(o + sizeof(int) * nw * RC_PTS);      // red_slot
    off[8] = o; o = RC_A16(o + (n <= RC_USED_LDS_MAX_N ? sizeof(unsigned) * ((n + 31) / 32) : 0));  // used (beyond: per-block global scratch)
    off[9] = o; o = RC_A16(o + sizeof(int) * 24);               // misc
    off[10] = o; o = RC_A16(o + sizeof(short) * kcap);         // act2
    off[11] = o; o = RC_A16(o + sizeof(short) * kcap);          // act
    off[12] = o; o = RC_A16(o + sizeof(int) * maxb);         // bx
    off[13] = o; o = RC_A16(o + sizeof(short) * maxb);       // ba
    off[14] = o; o = RC_A16(o + sizeof(short) * maxb);       // bb
    off[15] = o; o = RC_A16(o + sizeof(int) * (kcap + 1));      // seg
    off[16] = o; o = RC_A16(o + sizeof(unsigned short) * ((n + RC_PTS - 1) / RC_PTS + 1));  // ccnt
    off[17] = o; o = RC_A16(o + sizeof(int) * maxb);         // bu
    off[18] = o; o = RC_A16(o + sizeof(int) * maxb);         // blab
    off[19] = o; o = RC_A16(o + (size_t)kcap);                  // dirty
    off[20] = o; o = RC_A16(o + sizeof(short) * maxb);       // bK
    off[21] = o; o = RC_A16(o + (size_t)maxb);               // bflag
    off[22] = o; o = RC_A16(o + sizeof(short) * maxb);       // birth
    off[23] = o; o = RC_A16(o + sizeof(short) * 2 * maxb);   // pairs
    off[24] = o; o = RC_A16(o + (size_t)kcap);                  // candie
    off[25] = o; o = RC_A16(o + (kcap < 2048 ? (sizeof(int) + sizeof(short)) * RC_CPB_LDS * RC_PTS : 0));   // cu, cown (only below 2048 slots)
    off[26] = o; o = RC_A16(o + (size_t)kcap);                  // joined
    off[27] = o; o = RC_A16(o + sizeof(short) * 2 * maxb);   // pairs_tmp
    off[28] = o; o = RC_A16(o + 128 * 2 * sizeof(double));    // flt: the table of rc_flog, (double, double) entries (the score logarithms gather from it per lane)
    off[29] = o; o = RC_A16(o + (kcap < 2048 ? sizeof(double) * (kcap + 1) : 0));   // base_p (only below 2048 slots: the largest tables fill the CU as they are)
    return o;
}
