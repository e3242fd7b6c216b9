    const int outcome = run();
    const bool gaveUp = outcome == 1;
LFG_STAMP(
    const unsigned long long stampRunEnd = __builtin_amdgcn_s_memrealtime();
)
LFG_STAMP(
    if (lane == 0 && (fromQueue ? sp.units + unit : unit) < 8192) {
        unsigned long long *o = gMotionStamps + ((size_t)(fromQueue ? sp.units + unit : unit) * 4 + wave) * 8;
        o[0] = stampStart; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = stampEvals; o[3] = ((unsigned long long)borderTile << 32) | stampBatches | (((stampRunEnd - stampStart) & 0x3FFFFFFFull) << 33);
        o[4] = stampStaged; o[5] = stampFirst; o[6] = ((unsigned long long)stampBox << 32) | stampNarrow | (stampFour << 8) | ((unsigned long long)(fromQueue ? 1u : 0u) << 9) | ((unsigned long long)seg << 10) | ((unsigned long long)tileX << 12) | ((unsigned long long)tileY << 20);
        o[7] = ((unsigned long long)stampThrEnd << 32) | stampThr;
LFG_STAMP_PHASE(
        o[5] = (phaseLattice & 0xFFFFFull) | ((phaseSixteen & 0xFFFFFull) << 20) | ((phaseEval & 0xFFFFFull) << 40);
)
    }
)
    if (gaveUp) {
        // Flags live on the exact kernel's 64 x 64 tile grid (cleared before this launch): this tile spans
        // one or two of its columns.  Racing writers all store 1.  Sibling waves that already finished have
        // written their thresholds and counts; the resolve kernel ignores flagged tiles.
        if (lane == 0) {
            sGiveUp = 1u;
            const int ex0 = tx0 / kTW, ex1 = min(tx0 + kPTW - 1, W - 1) / kTW;
            // (the number of flagged tiles decides how the exact kernel shares them out; it follows the queue length;
            // the first kShareBelow of them are also listed, right behind the count)
            for (int ex = ex0; ex <= ex1; ++ex) {
                if (atomicExch(&tileFlags[tileY * flagTilesX + ex], 1u) == 0u) {
                    const uint32_t slot = atomicAdd(sp.queueCount + 1, 1u);
                    if (slot < (uint32_t)kShareBelow) sp.queueCount[2 + slot] = (uint32_t)(tileY * flagTilesX + ex);
                }
            }
        }
        if (!segUnit) return;              // (the waves of a segment unit meet at a barrier below)
    }
    if (outcome == 2) return;              // handed over (whole tiles only: no barrier below for them)
    // Threshold and count of every pixel, for the resolve kernel -- which never looks at a segment that settles all of
    // its pixels below, so such a segment (most of a frame under a pan) does not write them at all.
    auto writeThresholds = [&]() {
        // wave-uniform bases (whole tiles: the image-shaped arrays; shared tiles: the unit's private block) plus 32-bit lane
        // offsets, like the lists: a per-lane 64-bit pointer here was spilled, and its reload -- s_waitcnt vmcnt(0) --
        // made each of the 28 stores wait for the one before (20 us per wave that writes its thresholds)
        const size_t first = whole ? (size_t)(ty0 + kSeg * seg) * (size_t)W + (size_t)tx0
                                   : ((size_t)auxUnit * auxRows + (size_t)(kSeg * seg - auxRow0)) * (size_t)kPTW;
        float *const uBase = (whole ? uminOut : auxUminBase) + first;
        uint32_t *const cBase = (whole ? countOut : auxCountBase) + first;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int py = ty0 + kSeg * seg + 8 * hb + r8;
            const uint32_t off = (uint32_t)(8 * hb + r8) * rowStride + (uint32_t)(kRun * q);
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                if (!gaveUp && py < H && px0 + i < W && ((stripMask >> (kRun * hb + i)) & 1u) == 0u) {
                    const uint32_t cnt = (cnt2[hb][i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                    uBase[off + (uint32_t)i] = hb ? thr2[i].y : thr2[i].x;
                    cBase[off + (uint32_t)i] = cnt;
                }
            }
        }
    };
    const bool settlesHere = whole && !windowLeavesPrev;
    bool thresholdsNeeded = !settlesHere;  // (one call further down: the fourteen stores per lane are inlined once)
    // Whole tiles away from the rim settle their easy pixels here and now, while threshold and count are still in
    // registers: a zero-cost candidate (encoded in the threshold), a single record, or two records of which one
    // survives ARE the answer (motion_resolve_kernel's rules; no plateaus where the window stays inside prev).
    // A segment whose pixels were all settled says so, and the resolve kernel skips the blocks it covers.
    if (whole && !windowLeavesPrev) {
        // the first two records of the pixels that have any (a zero-cost pixel has none: most of a frame under a pan)
        const bool fastSettle = __builtin_amdgcn_readfirstlane((int)(allInside && settledAtZero)) != 0;
        Rec ra[2][kRun], rb[2][kRun];
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
            for (int i = 0; i < kRun; ++i) { ra[hb][i] = 0u; rb[hb][i] = 0u; }
        }
        if (!fastSettle) {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                const uint32_t cnt = (cnt2[hb][i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                if (cnt >= 1u) ra[hb][i] = waveList[laneOff[hb] + (uint32_t)i];
                if (cnt >= 2u) rb[hb][i] = waveList[rowStride + laneOff[hb] + (uint32_t)i];
            }
        }
        }
        uint32_t best[2][kRun];
        bool allSettled = true;
        if (fastSettle) {
            // the common case under a pan or where nothing moves: every threshold word IS the answer (rank + 0x00800000);
            // no records to look at, no pixel outside the image -- a dozen instructions instead of 250
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                const float fx = thr2[i].x, fy = thr2[i].y;            // (named floats: see refreshZeroBound)
                best[0][i] = __builtin_bit_cast(uint32_t, fx) - 0x00800000u;
                best[1][i] = __builtin_bit_cast(uint32_t, fy) - 0x00800000u;
            }
        } else
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int py = ty0 + kSeg * seg + 8 * hb + r8;
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                const float fx = thr2[i].x, fy = thr2[i].y;            // (named floats: see refreshZeroBound)
                const float bound = hb ? fy : fx;
                const uint32_t cnt = (cnt2[hb][i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                const bool inImage = py < H && px0 + i < W;
                const bool sa = rec_cost_low(ra[hb][i]) <= bound, sb = rec_cost_low(rb[hb][i]) <= bound;
                uint32_t b = 0xFFFFFFFFu;
                if (bound < 0.5f) b = __builtin_bit_cast(uint32_t, bound) - 0x00800000u;
                else if (cnt == 1u) b = rec_cand(ra[hb][i]);
                else if (cnt == 2u && sa != sb) b = sa ? rec_cand(ra[hb][i]) : rec_cand(rb[hb][i]);
                best[hb][i] = inImage ? b : 0xFFFFFFFFu;
                allSettled = allSettled && (!inImage || b != 0xFFFFFFFFu);
            }
        }
        // Only a segment that settles ALL of its pixels writes vectors (the resolve kernel redoes every pixel of any
        // other segment anyway), and it writes them as rows: the 16 x 56 vectors go through the wave's slab and leave
        // as 112 contiguous bytes per image row, two rows per store instruction -- a lane's own 2 x 7 pixels, stored
        // from where they were computed, touched sixteen cache lines per instruction with two bytes each (133 MB of
        // write requests per 4K frame for 16.6 MB of vectors).
        if (__builtin_amdgcn_readfirstlane(__ballot(!allSettled) == 0ull)) {
            uint16_t *const rows = reinterpret_cast<uint16_t *>(sSlab[wave]);          // [16][56] vectors (1,792 of 2,176 bytes)
            // (the lane number goes through an empty asm: the slab addresses derived from it are the same for every unit,
            //  and hoisted out of the workgroup's loop over units they are spilled and reloaded here behind a wait)
            int laneE = lane;
            asm volatile("" : "+v"(laneE));
            const int r8E = laneE & 7, qE = laneE >> 3;
            wave_lds_sync();
            // (all fourteen table reads first: interleaved with the slab stores -- through a generic pointer, which the
            //  compiler must assume may alias -- each read waited for the one before, fourteen L2 round trips in a row)
            int scanOf[2][kRun];
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
                for (int i = 0; i < kRun; ++i)
                    scanOf[hb][i] = (int)rank2scan[best[hb][i] != 0xFFFFFFFFu ? best[hb][i] : 0u];     // (outside the image: never stored)
            }
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
                for (int i = 0; i < kRun; ++i) {
                    const int scan = scanOf[hb][i];
                    const int dyi = scan / kSide, dxi = scan - dyi * kSide;
                    rows[(8 * hb + r8E) * kPTW + kRun * qE + i] = mv_word(dxi - kR, dyi - kR);
                }
            }
            wave_lds_sync();
            const bool wide = ((mvPitch & 3) == 0) && (((uintptr_t)mv & 3u) == 0u);       // 4-byte stores need 4-byte rows
            const int half = laneE / 28, d = laneE - half * 28;                          // 28 dwords = one row of the tile
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const int row = 2 * rr + half, py = ty0 + kSeg * seg + row, px = tx0 + 2 * d;
                if (laneE < 56 && py < H && px < W) {
                    const uint32_t two = *reinterpret_cast<const uint32_t *>(rows + row * kPTW + 2 * d);
                    if (kFused && sp.fused.data) {           // (wave-uniform) the north-star order: the generated pixels of these two vectors
                        fused_pixel(sp.fused, prev, prevPitch, curr, currPitch, W, H, px, py, (int)(int8_t)(two & 0xFFu), (int)(int8_t)((two >> 8) & 0xFFu));
                        if (px + 1 < W) fused_pixel(sp.fused, prev, prevPitch, curr, currPitch, W, H, px + 1, py, (int)(int8_t)((two >> 16) & 0xFFu), (int)(int8_t)(two >> 24));
                    }
                    int8_t *dst = mv + (size_t)py * (size_t)mvPitch + (size_t)px * 2u;
                    if (kFused && !sp.fused.storeMv) {
                    } else if (wide && px + 1 < W) *reinterpret_cast<uint32_t *>(dst) = two;
                    else {
                        *reinterpret_cast<uint16_t *>(dst) = (uint16_t)two;
                        if (px + 1 < W) *reinterpret_cast<uint16_t *>(dst + 2) = (uint16_t)(two >> 16);
                    }
                }
            }
            if (lane == 0) segDone[tile * (kPTH / kSeg) + seg] = 1u;
        } else {
            thresholdsNeeded = true;
        }
    }
    // (a segment unit whose four waves hold all parts of the order learns below whether any pixel is left to the resolve
    //  kernel; if none is -- most rim segments under a pan -- its 4 x 7 KB of thresholds and counts are never read: they were
    //  25 MB of the prefilter's 53 MB of writes per 4K frame, against 17 MB of vectors)
    const bool pooledUnit = LFG_LATE_THRESHOLDS && segUnit && nChunks == 4;
    if (thresholdsNeeded && !pooledUnit) writeThresholds();
    // A segment that is left to the resolve kernel goes onto its list, once: by the wave that owns it (whole tiles), by the
    // unit that holds the first part of the order (tiles shared between units), or -- segment units -- further down.
    if (thresholdsNeeded && !gaveUp && !segUnit && chunk == 0 && lane == 0)
        sp.openList[atomicAdd(sp.openCount, 1u)] = (uint32_t)(tile * (kPTH / kSeg) + seg);
    // (eight parts, two workgroups: no pooled settling below.  Plan units only: a handed-over segment was listed by the wave
    //  that pushed it -- listing it again here resolved it twice and could run past the list's tiles * 4 words)
    if (segUnit && nChunks != 4 && !fromQueue && !gaveUp && chunk == 0 && lane == 0)
        sp.openList[atomicAdd(sp.openCount, 1u)] = (uint32_t)(tile * (kPTH / kSeg) + seg);
    // A segment unit does the same for its segment, its four waves pooling what each learnt about its part of the
    // candidate order: the tightest threshold of the four is the pixel's bound, every wave holds its own records
    // against it, and a pixel with exactly one survivor among all four (or a zero-cost candidate) is settled --
    // unless the survivor stands for a plateau, which the resolve kernel sorts out.  The exchange goes through the
    // window's LDS, which every wave has finished with at the first barrier.
    if (segUnit && nChunks == 4) {         // (all parts of the order in this workgroup)
        constexpr int kPix = 2 * kRun * 64;                            // pixel slots of a wave (896)
        float *const sBound = reinterpret_cast<float *>(sWin);        // [4][kPix] thresholds
        uint32_t *const sMine = sWin + 4 * kPix;                       // [4][kPix] 0: no survivor, 0x80000000 | rank: one, ~0: unknown
        uint32_t *const sOpen = sWin + 8 * kPix;                       // some pixel of the segment is left to the resolve kernel
        static_assert(8 * kPix + 1 <= kWinH * kWinW, "exchange area fits the window");
        __syncthreads();
        if (*(volatile uint32_t *)&sGiveUp != 0u) return;              // the tile goes through the exact kernel
        Rec ra[2][kRun], rb[2][kRun];
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                const uint32_t cnt = (cnt2[hb][i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                ra[hb][i] = 0u; rb[hb][i] = 0u;
                if (cnt >= 1u) ra[hb][i] = waveList[laneOff[hb] + (uint32_t)i];
                if (cnt >= 2u) rb[hb][i] = waveList[rowStride + laneOff[hb] + (uint32_t)i];
                const float fx = thr2[i].x, fy = thr2[i].y;            // (named floats: see refreshZeroBound)
                sBound[wave * kPix + (kRun * hb + i) * 64 + lane] = hb ? fy : fx;
            }
        }
        if (tid == 0) *sOpen = 0u;
        __syncthreads();
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                const int at = (kRun * hb + i) * 64 + lane;
                const float bound = __builtin_fminf(__builtin_fminf(sBound[at], sBound[kPix + at]),
                                                    __builtin_fminf(sBound[2 * kPix + at], sBound[3 * kPix + at]));
                const uint32_t cnt = (cnt2[hb][i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                const bool sa = cnt >= 1u && rec_cost_low(ra[hb][i]) <= bound;
                const bool sb = cnt >= 2u && rec_cost_low(rb[hb][i]) <= bound;
                uint32_t word = 0u;
                if (cnt > 2u || (sa && sb)) word = 0xFFFFFFFFu;
                else if (sa) word = 0x80000000u | rec_cand(ra[hb][i]);
                else if (sb) word = 0x80000000u | rec_cand(rb[hb][i]);
                sMine[wave * kPix + at] = word;
            }
        }
        __syncthreads();
        // (three passes over this wave's share of the fourteen slots -- decide, read the table, store -- so that the table
        //  reads are in flight together: read and stored slot by slot, each read waited for the store before it)
        bool open = false;
        uint32_t bestOf[2][kRun];
        bool singleOf[2][kRun];
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int py = ty0 + kSeg * seg + 8 * hb + r8;
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                bestOf[hb][i] = 0xFFFFFFFFu; singleOf[hb][i] = false;
                if (((kRun * hb + i) & 3) != wave) continue;           // the fourteen slots are dealt out to the four waves
                if (!(py < H && px0 + i < W) || ((stripMask >> (kRun * hb + i)) & 1u) != 0u) { bestOf[hb][i] = 0xFFFFFFFEu; continue; }      // (outside the image, or the strip kernel's: nothing to do)
                const int at = (kRun * hb + i) * 64 + lane;
                const float bound = __builtin_fminf(__builtin_fminf(sBound[at], sBound[kPix + at]),
                                                    __builtin_fminf(sBound[2 * kPix + at], sBound[3 * kPix + at]));
                if (bound < 0.5f) {
                    bestOf[hb][i] = __builtin_bit_cast(uint32_t, bound) - 0x00800000u;
                } else {
                    uint32_t n = 0u, any = 0u;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const uint32_t word = sMine[w * kPix + at];
                        n += word != 0u ? 1u : 0u;
                        any |= word;
                    }
                    // exactly one wave reports, and it reports a single rank
                    if (n == 1u && any != 0xFFFFFFFFu) { bestOf[hb][i] = any & 0x7FFFFFFFu; singleOf[hb][i] = true; }
                }
            }
        }
        int scanOfSeg[2][kRun];
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                scanOfSeg[hb][i] = 0;
                if (((kRun * hb + i) & 3) != wave) continue;
                scanOfSeg[hb][i] = (int)rank2scan[bestOf[hb][i] < (uint32_t)kCand ? bestOf[hb][i] : 0u];
            }
        }
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int py = ty0 + kSeg * seg + 8 * hb + r8;
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
                if (((kRun * hb + i) & 3) != wave) continue;
                if (bestOf[hb][i] == 0xFFFFFFFEu) continue;            // outside the image
                bool settled = bestOf[hb][i] != 0xFFFFFFFFu;
                if (settled) {
                    const int scan = scanOfSeg[hb][i];
                    const int dyi = scan / kSide, dxi = scan - dyi * kSide;
                    if (singleOf[hb][i] && block_leaves_prev(px0 + i, py, dxi - kR, dyi - kR, W, H)) settled = false;
                    if (settled) {
                        if (kFused && sp.fused.data) fused_pixel(sp.fused, prev, prevPitch, curr, currPitch, W, H, px0 + i, py, dxi - kR, dyi - kR);
                        int8_t *dst = mv + (size_t)py * (size_t)mvPitch + (size_t)(px0 + i) * 2u;
                        if (!kFused || sp.fused.storeMv)
                        *reinterpret_cast<uint16_t *>(dst) = mv_word(dxi - kR, dyi - kR);   // both components, one store
                    }
                }
                open = open || !settled;
            }
        }
        if (__builtin_amdgcn_readfirstlane(__ballot(open) != 0ull) && lane == 0) *sOpen = 1u;
        __syncthreads();
        if (tid == 0) {
            if (*sOpen == 0u) segDone[tile * (kPTH / kSeg) + seg] = 1u;
            else sp.openList[atomicAdd(sp.openCount, 1u)] = (uint32_t)(tile * (kPTH / kSeg) + seg);
        }
        if (pooledUnit && *(volatile uint32_t *)sOpen != 0u) writeThresholds();
    }
LFG_STAMP(
    if (lane == 0 && (fromQueue ? sp.units + unit : unit) < 8192)      // (the end of the unit with its epilogue)
        gMotionStamps[((size_t)(fromQueue ? sp.units + unit : unit) * 4 + wave) * 8 + 1] = __builtin_amdgcn_s_memrealtime();
)
