        // ---- Narrow search.  A segment that holds pixels without any match searches in full: no test can drop a
        // candidate for the whole wave, and every candidate costs a full evaluation of all 16 x 56 pixels although only
        // the unmatched ones can still record anything.  Often those lie in a narrow band of columns -- the strip a pan
        // exposes at the left or right edge (ten columns for the benchmark's motion), the vertical edge of a moving
        // object or of an occlusion: two thirds of the full-search waves on the benchmark's pan, a fifth to a third on
        // the occluded and moving-object frames.  Once the hints have been tried the wave looks at its thresholds: if
        // every pixel that is still above LFG_NARROW_THR lies within W <= 16 columns (W a multiple of four), those
        // columns leave the wide machinery -- their thresholds and counts move to LDS, the registers hold -inf, which
        // never passes a test and does not count in waveThr, so the lattice tests work again for the rest of the
        // segment -- and are searched AFTER the wide batches, K = 64 / (W + 8) candidates per pass (5 | 4 | 3 | 2):
        //   * lanes (candidate k, position column j) compute the band's W + 7 position columns for K candidates side
        //     by side: window reads, distances and column sums are the wide code with per-lane offsets;
        //   * the slab holds all sixteen rows (pitch 164, columns interleaved four ways: writes and reads conflict-free);
        //   * lanes (pixel row, group of four columns) then take the K candidates one after the other: eleven reads,
        //     22 adds, four comparisons each, with the pixel's threshold, count and list handled by this one lane as
        //     in the wide code -- nothing shared, no atomics.
        // Distances and column sums, two thirds of an evaluation, are paid once per K candidates, the row sums cover
        // 16 x W pixels instead of 16 x 56.  At the end thresholds and counts go back to the lanes that own the pixels
        // in the wide layout and the epilogue runs unchanged.
        // (After the wide batches, not between them: by then the wide machinery's registers -- the lane's 23
        //  current-frame texels and their squares above all -- are free.  Interleaved, the two sets did not fit and
        //  every pass waited for scratch reloads behind its own record stores.)
        bool narrow = false;
        int nXb = 0, nW = 0;                                           // the band: pixel columns nXb .. nXb + nW - 1 of the tile
        uint32_t *const nThr = sNarrow[wave];                          // [16][kNarrowMax] threshold words (float bits)
        uint32_t *const nCnt = nThr + kSeg * kNarrowMax;               // [16][kNarrowMax] records so far | plateau member seen << 31
        auto entryOf = [&](int idx) { return min(idx < nHead ? idx : eBegin + (idx - nHead), kCand - 1); };
        auto enterNarrow = [&]() {
            int lo = 99, hi = -1;
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                const float fx = thr2[i].x, fy = thr2[i].y;            // (-inf: outside the image; +inf: nothing yet)
                if (fx >= LFG_NARROW_THR || fy >= LFG_NARROW_THR) { lo = min(lo, kRun * q + i); hi = max(hi, kRun * q + i); }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_xor(lo, off)); hi = max(hi, __shfl_xor(hi, off)); }
            lo = __builtin_amdgcn_readfirstlane(lo); hi = __builtin_amdgcn_readfirstlane(hi);
            if (hi < lo || hi - lo >= kNarrowMax) return;
            nW = ((hi - lo) / 4 + 1) * 4;
            nXb = min(lo, kPTW - nW);
            wave_lds_sync();
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
                for (int i = 0; i < kRun; ++i) {
                    const int col = kRun * q + i - nXb;
                    if (col >= 0 && col < nW) {
                        const int cell = (8 * hb + r8) * kNarrowMax + col;
                        const float fx = thr2[i].x, fy = thr2[i].y;
                        nThr[cell] = __builtin_bit_cast(uint32_t, hb ? fy : fx);
                        nCnt[cell] = ((cnt2[hb][i >> 1] >> (16 * (i & 1))) & 0xFFFFu) | (((plateauSeen >> (kRun * hb + i)) & 1u) << 31);
                        if (hb) thr2[i].y = -__builtin_inff(); else thr2[i].x = -__builtin_inff();
                    }
                }
            }
            wave_lds_sync();
            narrow = true;
LFG_STAMP(
            stampNarrow = (unsigned)(64 / ((nW + kB - 1 + 3) & ~3));
)
        };
        auto narrowPhase = [&](int iBegin) -> bool {
            const int iEnd = nEntries;
            const int groups = nW / 4;
            const int colsPer = (nW + kB - 1 + 3) & ~3;                // 12 | 16 | 20 | 24 slab columns per candidate
            const int perPass = 64 / colsPer;                          // 5 | 4 | 3 | 2 candidates
            // compute side: lane = (candidate kc, position column nXb + cl); spare lanes repeat the last one
            int kc = lane / colsPer, cl = lane - kc * colsPer;
            if (kc >= perPass) { kc = perPass - 1; cl = colsPer - 1; }
            const int pcol = min(nXb + cl, kPTW + kB - 2);             // (the padding columns of a candidate compute sums nobody reads)
            const lds_ro_u32_ptr nWin = (lds_ro_u32_ptr)(sWin + pcol * kWinH + kSeg * seg);
            uint32_t cN[kSegD], ccN[kSegD], nValid = 0u;
            {
                const int gx = bx0 + pcol;
                const bool okx = gx >= 0 && gx < W;
                const uint8_t *const column = curr + (size_t)clampi(gx, 0, W - 1) * 4u;
                // (the pitch through an empty asm: sharing the 23 row offsets with the loads at the unit's start keeps 46
                //  scalars alive -- spilled -- from there to here in every unit, narrow or not)
                int pitchN = currPitch;
                asm volatile("" : "+s"(pitchN));
#pragma unroll
                for (int j = 0; j < kSegD; ++j) {
                    const int gy = by0 + kSeg * seg + j;
                    const bool ok = okx && gy >= 0 && gy < H;
                    const uint32_t t = *reinterpret_cast<const uint32_t *>(column + (size_t)clampi(gy, 0, H - 1) * (size_t)pitchN);
                    cN[j] = ok ? t : 0u;
                    nValid |= (ok ? 1u : 0u) << j;
                }
#pragma unroll
                for (int j = 0; j < kSegD; ++j) ccN[j] = __builtin_amdgcn_udot4(cN[j], cN[j], 0x4B000000u, false);
            }
            f32x2 *const nSlabW = reinterpret_cast<f32x2 *>(sSlab[wave]) + ((lane & 3) * kNarrowQ + (lane >> 2));    // slab column = lane
            // read side: lane = (pixel row r, group g of four columns)
            const int r = lane & 15, g = lane >> 4;
            const bool active = g < groups;
            float thrN[4];
            uint32_t cntN[4], platN = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cell = r * kNarrowMax + 4 * (active ? g : 0) + j;
                const uint32_t w = nCnt[cell];
                thrN[j] = active ? __builtin_bit_cast(float, nThr[cell]) : -__builtin_inff();
                cntN[j] = w & 0xFFFFu;
                platN |= (w >> 31) << j;
            }
            // column sum i (0..10) of candidate k for this lane: slab column c = colsPer k + 4 g + i, stored at (c & 3) kNarrowQ + c / 4
            const lds_ro_f32_ptr nSlabR = (lds_ro_f32_ptr)(sSlab[wave] + (r >> 1) * kNarrowPitch + (r & 1) + 2 * (active ? g : 0));
            const uint32_t nLaneOff = (uint32_t)r * (listK * rowStride) + (uint32_t)(nXb + 4 * g);
            const int segY0 = ty0 + kSeg * seg;
            // (A candidate no lane records -- nearly every one of the 1,089 -- costs the slab reads, the tree, the compare and
            //  ONE branch on the ballot itself.  Its entry of the order and all that derives from it are the hit side's business:
            //  fetched in front of the branch, the entry was an LDS round trip, a readfirstlane and a dozen scalar instructions
            //  per candidate, and the ballot wrapped in a readfirstlane went through a select, a lane read and a bit test
            //  before it could branch -- 71 instructions on that path, 46 now: tools/full_search_budget.py.)
            auto testCandidate = [&](const float (&X)[4 + kB - 1], int idx) {
                float h2[10], h4[8], sN[4];
#pragma unroll
                for (int i = 0; i < 10; ++i) h2[i] = X[i] + X[i + 1];
#pragma unroll
                for (int i = 0; i < 8; ++i) h4[i] = h2[i] + h2[i + 2];
#pragma unroll
                for (int i = 0; i < 4; ++i) sN[i] = h4[i] + h4[i + 4];
                float top = thrN[0] - sN[0];
#pragma unroll
                for (int j = 1; j < 4; ++j) top = __builtin_fmaxf(top, thrN[j] - sN[j]);
                if (__ballot(top >= 0.0f) == 0ull) return;
                const uint32_t ord = (uint32_t)__builtin_amdgcn_readfirstlane((int)((lds_ro_u32_ptr)sOrder)[entryOf(idx)]);
                const uint32_t countIt = idx >= nHead ? 1u : 0u;
                const uint32_t cand = ord & 0xFFFFu;
                const int candDx = (int)((ord >> 16) / (uint32_t)kWinH) - kR, candDy = (int)((ord >> 16) % (uint32_t)kWinH) - kR;
                const uint32_t zeroCap = 0x00800000u + cand;
                const bool candMayLeave = windowLeavesPrev &&
                    block_leaves_prev_any(tx0 + nXb, min(tx0 + nXb + nW - 1, W - 1), segY0, min(segY0 + kSeg - 1, H - 1), candDx, candDy, W, H);
                unsigned long long hit[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) hit[j] = __ballot(sN[j] <= thrN[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (hit[j] != 0ull) {                              // wave-uniform
                        asm volatile("; some lane records a candidate (narrow)");
                        const float s = sN[j];
                        if (s <= thrN[j]) {                            // (the rules of rowSumsAndTest)
                            const float cap = __builtin_fmaxf(s * kRatio, __builtin_bit_cast(float, zeroCap));
                            if (s < thrN[j] * kRestart) cntN[j] = 0u;   // (`restart`: every earlier record is dead)
                            thrN[j] = __builtin_fminf(thrN[j], cap);
                            const uint32_t at = __umul24(min(cntN[j], listK - 1u), rowStride) + nLaneOff + (uint32_t)j;
                            if (s != 0.0f) waveList[at] = rec_make(s, cand);
                            uint32_t inc = (s != 0.0f && countIt != 0u) ? 1u : 0u;
                            if (candMayLeave) {
                                uint32_t l;
                                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=&v"(l));
                                const bool plateau = block_leaves_prev(tx0 + nXb + 4 * (int)(l >> 4) + j, segY0 + (int)(l & 15u), candDx, candDy, W, H);
                                inc = (plateau && ((platN >> j) & 1u) != 0u) ? 0u : inc;
                                platN |= (plateau && inc != 0u) ? (1u << j) : 0u;
                            }
                            cntN[j] += inc;
                        }
                    }
                }
            };
            uint32_t p[kSegD];
            f32x2 c8[8];
            float v8[kSeg];
            bool pending = false;
            int idx0 = iBegin, idxP = 0, started = 0;
            // (as in the row band: a lane's entry of the order is fetched a pass ahead -- fetched where it is needed, it was an LDS
            //  round trip of its own in front of the window reads.  The row band's other idiom, the previous pass's first slab
            //  reads BEFORE the window reads, costs eleven live registers across the 23 window reads here: vgpr_spill_count 6 -> 14.)
            auto orderAt = [&](int idx) { return ((lds_ro_u32_ptr)sOrder)[entryOf(min(idx + kc, iEnd - 1))]; };
            auto slabReads = [&](int k, float (&X)[4 + kB - 1]) {
                const lds_ro_f32_ptr base = nSlabR + 2 * (colsPer / 4) * k;
#pragma unroll
                for (int i = 0; i < 4 + kB - 1; ++i) X[i] = base[2 * ((i & 3) * kNarrowQ + (i >> 2))];
            };
            uint32_t ordN = orderAt(idx0);
            for (;;) {
                const bool have = idx0 < iEnd && started < 64;
                if (!have && !pending) {                               // (the pipeline has drained) every 64 entries: give up?
                    if (idx0 >= iEnd) break;
                    started = 0;
                    const bool over = cntN[0] >= listK || cntN[1] >= listK || cntN[2] >= listK || cntN[3] >= listK;    // (the last slot is a spare)
                    if (__ballot(over) != 0ull) sGiveUp = 1u;
                    if (unitGaveUp()) return false;
                    continue;
                }
                if (have) {
                    const lds_ro_u32_ptr w = nWin + (ordN >> 16);
#pragma unroll
                    for (int j = 0; j < kSegD; ++j) p[j] = w[j];
                    ordN = orderAt(idx0 + perPass);
                }
                if (pending) {             // the slab holds the previous pass: sixteen rows of perPass candidates' column sums
                    wave_lds_sync();
#pragma nounroll                   // (one copy of the test, not one per candidate)
                    for (int k = 0, kEnd = min(perPass, iEnd - idxP); k < kEnd; ++k) {
                        float X[4 + kB - 1];
                        slabReads(k, X);
                        testCandidate(X, idxP + k);
                    }
                    wave_lds_sync();
                }
                __builtin_amdgcn_sched_barrier(0);
                if (have) {
                    columnSums(p, cN, ccN, nValid, c8);
#pragma unroll
                    for (int a = 0; a < 8; ++a) { v8[a] = c8[a].x; v8[a + 8] = c8[a].y; }
                    wave_lds_sync();
#pragma unroll
                    for (int a = 0; a < 8; ++a) nSlabW[a * (kNarrowPitch / 2)] = f32x2{v8[2 * a], v8[2 * a + 1]};
                    wave_lds_sync();
                    started += perPass;
                }
                idxP = idx0; pending = have;
                if (have) idx0 += perPass;
            }
            // the band's final thresholds and counts: through LDS back to the lanes that own the pixels in the wide layout
            wave_lds_sync();
            if (active) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int cell = r * kNarrowMax + 4 * g + j;
                    nThr[cell] = __builtin_bit_cast(uint32_t, thrN[j]);
                    nCnt[cell] = min(cntN[j], 0x7FFFu) | (((platN >> j) & 1u) << 31);
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
                for (int i = 0; i < kRun; ++i) {
                    const int col = kRun * q + i - nXb;
                    if (col >= 0 && col < nW) {
                        const int cell = (8 * hb + r8) * kNarrowMax + col;
                        const float t = __builtin_bit_cast(float, nThr[cell]);
                        const uint32_t w = nCnt[cell];
                        if (hb) thr2[i].y = t; else thr2[i].x = t;
                        const uint32_t sh = 16u * (uint32_t)(i & 1);
                        cnt2[hb][i >> 1] = (cnt2[hb][i >> 1] & ~(0xFFFFu << sh)) | ((w & 0xFFFFu) << sh);
                        plateauSeen |= (w >> 31) << (kRun * hb + i);
                    }
                }
            }
            return true;
        };
