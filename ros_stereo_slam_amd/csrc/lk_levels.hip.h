// lk_levels.hip.h -- the level loop of lk_track_kernel (lk.hip), included INSIDE the kernel once per body: the including
// block defines `constexpr int CA` (channels of arithmetic per pixel), `CS` (channels per pixel of the levels it stages: the
// kernel's C, or 1 for the grey regions of grey-stored three-channel pyramids) and `MUL = C / CA`,
// everything else is the kernel's own scope.  Text instead of a lambda or a function template on purpose: wrapped in
// either, the same statements compiled to 2 to 4 more registers in EVERY instantiation (66 / 70 instead of 64 / 70 at
// C == 1, 98 / 102 instead of 96 / 100 at C == 3), which costs the three-channel kernels their fifth wave per SIMD.
// No include guard: it is meant to be included more than once.
    for (int level = prm.max_level; level >= 0; level--) {
        const int lw = prev.w[level], lh = prev.h[level];
        // CS == C: the pyramids' own levels; CS = 1 with C = 3: the grey regions of two grey-stored pyramids, a one-channel
        // pyramid's layout (svo_internal.h)
        const uint8_t *I = CS == C ? prev.lvl[level] : prev.lvl[level] + prm.gdelta[level];
        const uint8_t *J = CS == C ? next.lvl[level] : next.lvl[level] + prm.gdelta[level];
        const int pitch = CS == C ? prev.pitch[level] : svo_grey_pitch(lw);
        const int *dlevel = dprev + (CS == C ? prm.doff[level] : prm.gdoff[level]);
        const int dpitch = CS == C ? prm.dpitch[level] : svo_grey_dpitch(lw);
        constexpr int TROW = Tile<CS, PT>::ROW;
        const float scale = 1.f / (float)(1 << level);
        float px = ptx * scale, py = pty * scale;
        float nxp, nyp;
        if (level == prm.max_level) {
            nxp = px;
            nyp = py;
        } else {
            nxp = outx * 2.f;
            nyp = outy * 2.f;
        }
        outx = nxp;
        outy = nyp;
        px -= half;
        py -= half;
        const int ipx = uniform_int_of(floorf(px)), ipy = uniform_int_of(floorf(py));
        if (ipx < -WIN || ipx >= lw || ipy < -WIN || ipy >= lh) {
            if (level == 0) {
                st = 0;
                errv = 0.f;
            }
            continue;
        }
        // ---- 1. previous-image tile -> template patch; derivative tile -> derivative patches, normal matrix ----
        // Both tiles' loads are issued at once: T is written to LDS as soon as it has arrived, the eight vectors
        // of D stay in flight (in registers) while the template patch is formed from T, and take T's place after.
        //
        // A window that starts on an integer position (both fractions exactly 0: the lattice points of a keyframe at
        // the levels whose scale divides the grid step) has the weights (2^14, 0, 0, 0), and the interpolation is the
        // identity:  (2^14 p + 2^8) >> 9 == 32 p  and  (2^14 4d + 4 2^13) >> 16 == d.  Such a level unpacks what it
        // staged instead of interpolating it (IDENT): the same patches bit for bit, a quarter of the instructions.
        // The choice is the kernel's own, from the fractions, valid for any point; it is made BEFORE the loads are
        // issued, so that no branch falls inside the window in which the loads are in flight.
        const float fa = px - (float)ipx, fb = py - (float)ipy;
        int Ivp[npairs(CA)], Ixp[npairs(CA)], Iyp[npairs(CA)];  // packed int16 pairs (low = even element)
        auto patches = [&](auto ident_c) {
            constexpr bool IDENT = decltype(ident_c)::value;
            constexpr int NE = SEG * CA, NV = (SEG + 1) * CA;
            int wv0 = 0, wv1 = 0;  // (w00 | w10 << 16), (w01 | w11 << 16)
            if constexpr (!IDENT) {
                int w00, w01, w10, w11;
                bilinear_weights(fa, fb, w00, w01, w10, w11);
                wv0 = (w00 & 0xffff) | (w10 << 16);
                wv1 = (w01 & 0xffff) | (w11 << 16);
            }
            wave_lds_sync();
            TileLoad<CS, PT> tload;
            tile_issue<CS, PT>(tload, I, pitch, ipx - 1, ipy - 1, lane);
            DtileLoad<CS> dload;
            dtile_issue<CS>(dload, dlevel, dpitch, ipx, ipy, lane);
            tile_commit<CS, PT, DtileLoad<CS>::N>(tload, T, lane);
            const uint8_t *Ts = T + tload.shift;
            wave_lds_sync();

            const int toff = (int)(Ts - lds) + (wy + 1) * TROW + (wx + 1) * CS;
            if constexpr (IDENT) {
                // element k is its byte of the lane's row run, times 32: one permute spreads two bytes over the
                // halves of a dword, one shift scales both (32 * 255 stays inside its half)
                unsigned t0[ndwords(CS)];
                load_row_packed<CS>(lds, toff, t0);
                ForEachElem<CA, npairs(CA)>::run([&](auto jc) {
                    constexpr int j = decltype(jc)::value, k0 = 2 * j, k1 = 2 * j + 1;
                    constexpr int b0 = elem_at(k0, CA, CS), b1 = elem_at(k1 < NE ? k1 : k0, CA, CS);  // their bytes
                    constexpr unsigned hi = k1 < NE ? 4u + (unsigned)(b1 & 3) : 0x0cu;
                    constexpr unsigned sel = (unsigned)(b0 & 3) | (0x0cu << 8) | (hi << 16) | (0x0cu << 24);
                    Ivp[j] = (int)(__builtin_amdgcn_perm(t0[b1 >> 2], t0[b0 >> 2], sel) << 5);
                });
            } else {
                unsigned t0[ndwords(CS)], t1[ndwords(CS)];
                load_row_packed<CS>(lds, toff, t0);
                load_row_packed<CS>(lds, toff + TROW, t1);
                lane_samples<CA, CS, W_BITS - 5>(t0, t1, wv0, wv1, Ivp);
            }
            // the Scharr derivatives of the window's 22x22 neighbourhood come from the derivative level
            // (zero outside the image: the level's border is zero); the tile takes the place of T.
            // The template patch is finished before the staging starts: its operands are inputs of the asm that
            // hands the staging its lane index (otherwise the compiler carries raw tile rows across the loads).
            int dl = lane;
            static_assert(npairs(CA) == 11 || npairs(CA) == 4, "list the template registers below");
            if constexpr (npairs(CA) == 11)
                asm volatile("" : "+v"(dl) : "v"(Ivp[0]), "v"(Ivp[1]), "v"(Ivp[2]), "v"(Ivp[3]), "v"(Ivp[4]), "v"(Ivp[5]),
                             "v"(Ivp[6]), "v"(Ivp[7]), "v"(Ivp[8]), "v"(Ivp[9]), "v"(Ivp[10]));
            else
                asm volatile("" : "+v"(dl) : "v"(Ivp[0]), "v"(Ivp[1]), "v"(Ivp[2]), "v"(Ivp[3]));
            wave_lds_sync();
            dtile_commit<CS>(dload, DB, dl);
            const int *D = reinterpret_cast<const int *>(DB + dload.shift);
            wave_lds_sync();
            constexpr int DROW = DTile<CS>::ROW / 4;
            int dlane = wy * DROW + wx * CS;  // this lane's first tile entry
            // Derivative tile entries are (4 dx | 4 dy << 16) (pyramid.hip; |4 d| <= 16320: int16).
            if constexpr (IDENT) {
                // element k is its entry of the lane's row run: the low (x) / high (y) halves of two entries packed by
                // one permute, the factor 4 dropped by one packed arithmetic shift.  The spare lane (63) selects
                // zero bytes: Ix = Iy = 0 there, as its zero weights give in the interpolating path.
                const int *d0 = D + dlane;
                int e[NE + 1];
#pragma unroll
                for (int k = 0; k < NE; k++)
                    e[k] = d0[elem_at(k, CA, CS)];
                e[NE] = 0;
                // (The selectors do not depend on the level.  Left to itself the compiler forms them once, before
                // the level loop, and keeps them and their constants in registers across the iteration loop, which
                // has none to spare: so from an opaque copy of the lane, the constants as literals of the VOP2 forms.)
                int sl = lane;
                asm volatile("" : "+v"(sl));
                const int spare = sl < 3 * WIN ? 0 : -1;
                unsigned selx, sely;  // 0x05040100 / 0x07060302: the low / high halves of two dwords; 0x0c: a zero byte
                asm("v_and_b32 %0, 0x09080d0c, %1\n\tv_xor_b32 %0, 0x05040100, %0" : "=v"(selx) : "v"(spare));
                asm("v_and_b32 %0, 0x0b0a0f0e, %1\n\tv_xor_b32 %0, 0x07060302, %0" : "=v"(sely) : "v"(spare));
                const short2v two = {2, 2};
#pragma unroll
                for (int j = 0; j < npairs(CA); j++) {
                    const unsigned lo = (unsigned)e[2 * j], hi = (unsigned)e[2 * j + 1 < NE ? 2 * j + 1 : NE];
                    Ixp[j] = __builtin_bit_cast(int, (short2v)(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(hi, lo, selx)) >> two));
                    Iyp[j] = __builtin_bit_cast(int, (short2v)(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(hi, lo, sely)) >> two));
                }
            } else {
                // As for the image samples, the VERTICAL neighbours of column k are paired once (element k uses
                // columns k and k + C): 2 permutes per column instead of 4 per element.  With the factor 4 the
                // descale by 2^14 is "take the high half" -- the permute that packs two elements does it, no shift:
                //   (4 (sum w d) + 4 RD) >> 16  ==  (sum w d + RD) >> 14.
                constexpr int RD4 = 4 << (W_BITS - 1);
                // the spare lane (63) interpolates its derivative patch with zero weights: Ix = Iy = 0 there, so
                // its share of every sum below and in the iterations is 0 without any masking
                const int wq0 = active ? wv0 : 0, wq1 = active ? wv1 : 0;
                // x then y, each from its own read of the tile rows: half the registers in flight
                {
                    const int *d0 = D + dlane, *d1 = d0 + DROW;
                    int vx[NV], sx[NE + 1];
                    ForEachElem<CA, NV>::run([&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        vx[k] = half_pair<false>(d0[elem_at(k, CA, CS)], d1[elem_at(k, CA, CS)]);
                    });
                    sx[NE] = 0;
#pragma unroll
                    for (int k = 0; k < NE; k++)
                        sx[k] = sdot2(vx[k + CA], wq1, sdot2_sconst(vx[k], wq0, RD4));
#pragma unroll
                    for (int j = 0; j < npairs(CA); j++)
                        Ixp[j] = half_pair<true>(sx[2 * j], sx[2 * j + 1 < NE ? 2 * j + 1 : NE]);
                }
                // the y pass starts when the x pass is done (left alone the compiler merges the two and needs 106
                // registers; at most 104 keep a fifth wave slot's worth of every SIMD free for the short kernels)
                asm volatile("" : "+v"(dlane), "+v"(Ixp[npairs(CA) - 1]));
                {
                    const int *d0 = D + dlane, *d1 = d0 + DROW;
                    int vy[NV], sy[NE + 1];
                    ForEachElem<CA, NV>::run([&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        vy[k] = half_pair<true>(d0[elem_at(k, CA, CS)], d1[elem_at(k, CA, CS)]);
                    });
                    sy[NE] = 0;
#pragma unroll
                    for (int k = 0; k < NE; k++)
                        sy[k] = sdot2(vy[k + CA], wq1, sdot2_sconst(vy[k], wq0, RD4));
#pragma unroll
                    for (int j = 0; j < npairs(CA); j++)
                        Iyp[j] = half_pair<true>(sy[2 * j], sy[2 * j + 1 < NE ? 2 * j + 1 : NE]);
                }
            }
        };
        if (prm.lattice && uniform(fa == 0.f && fb == 0.f))
            patches(std::true_type());
        else
            patches(std::false_type());
        int a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
        for (int j = 0; j < npairs(CA); j++) {
            a11 = sdot2(Ixp[j], Ixp[j], a11);  // sums of squares of int16 pairs, exact
            a12 = sdot2(Ixp[j], Iyp[j], a12);
            a22 = sdot2(Iyp[j], Iyp[j], a22);
        }
        int neg_c1 = 0, neg_c2 = 0;  // - sum I * Ix, - sum I * Iy of this lane (see lane_mismatch)
#pragma unroll
        for (int j = 0; j < npairs(CA); j++) {
            neg_c1 = sdot2(Ivp[j], Ixp[j], neg_c1);
            neg_c2 = sdot2(Ivp[j], Iyp[j], neg_c2);
        }
        neg_c1 = -neg_c1;
        neg_c2 = -neg_c2;
        // The template patch has one use left, the level-0 residual after the iterations.  At C = 3 it waits for it in the
        // LDS the J tile leaves free (the wave's area is sized by the derivative tile, which is consumed by now) instead
        // of in 11 registers the iteration loop needs: lane l's dwords at PARK + 4 l + 256 k, conflict-free.
        constexpr bool PARK_IVP = WANT_ERR && CA == 3;
        constexpr int PARK = Tile<C, TS>::BYTES;
        static_assert(!PARK_IVP || PARK + npairs(CA) * 256 <= Lds<C>::WAVE_BYTES, "no room for the parked template patch");
        if constexpr (PARK_IVP) {
            if (level == 0) {
                wave_lds_sync();
                int *park = reinterpret_cast<int *>(lds + PARK) + lane;
#pragma unroll
                for (int k = 0; k < npairs(CA); k++)
                    park[64 * k] = Ivp[k];
            }
        }
        float A11, A12, A22;
        wave_sum3_float<MUL>(a11, a12, a22, A11, A12, A22);
        A11 *= FLT_SCALE;
        A12 *= FLT_SCALE;
        A22 *= FLT_SCALE;
        float Dd = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) /
                             (float)(2 * WIN * WIN);
        if (level == 0)
            mineig0 = minEig;
        if (uniform(minEig < prm.min_eig_thr || Dd < 1.1920928955078125e-7f)) {
            if (level == 0)
                st = 0;
            continue;
        }
        Dd = 1.f / Dd;
        // The reference scales the mismatch sums by 2^-20 before the 2x2 solve.  A power of two commutes with
        // every rounding of  (A12 b2 - A22 b1) Dd  (no overflow: |b| < 2^31, no underflow: Dd <= 8.4e6 and the
        // difference is a multiple of an ulp of its terms), so it is applied to Dd once per level instead of to
        // both sums in every iteration: the same step bit for bit.
        const float Dds = Dd * FLT_SCALE;

        // ---- 2. iterate on the next image out of an LDS tile ----
        nxp -= half;
        nyp -= half;
        float pdx = 0.f, pdy = 0.f;
        const int lane_off = wy * Tile<CS, TS>::ROW + wx * CS;  // this lane's row run inside the window
        int ox = 0, oy = 0;
        bool have_tile = false;
        int tj_off = 0;          // LDS byte offset of the staged tile's pixel (0, 0): TJ's offset + the staging shift
        bool stepped = false;    // at least one Newton step taken: the output is nxp + half (else the guess itself)
        bool out_set = false;    // left through the oscillation test: the output (backed off half a step) is written there
        // The iterations of a level, as passes over pixel cells: the column pairs of the lane's two row runs depend on
        // the staged tile and on the guess's integer cell (inx, iny) only, so the inner loop keeps them in registers
        // and goes on for as long as the guess stays in its cell (after the first step of a level: about every
        // second iteration).  A guess that leaves the cell returns to the outer loop, which re-stages the tile when
        // the guess has drifted off it and loads and pairs the rows of the new cell.  Wave-uniform integers: scalar
        // compares and scalar branches.  With prm.cell_cache == 0 every iteration returns to the outer loop.
        float fx = floorf(nxp), fy = floorf(nyp);
        int inx = uniform_int_of(fx), iny = uniform_int_of(fy);
        bool more = prm.max_count > 0;
        if (more && (inx < -WIN || inx >= lw || iny < -WIN || iny >= lh)) {
            if (level == 0)
                st = 0;
            more = false;
        }
        int j = 0;
        while (more) {
            if (!have_tile || inx < ox || inx > ox + 2 * JR || iny < oy || iny > oy + 2 * JR) {
                ox = inx - JR;
                oy = iny - JR;
                wave_lds_sync();
                tj_off = (int)(TJ - lds) + uniform(stage_tile<CS, TS>(TJ, J, pitch, ox, oy, lane));
                wave_lds_sync();
                have_tile = true;
            }
            int V[(SEG + 1) * CA];
            lane_load_pairs<CA, CS>(lds, lane_off + (tj_off + (iny - oy) * Tile<CS, TS>::ROW + (inx - ox) * CS), V);
            const int cx = inx, cy = iny;
            for (;;) {
                int wv0, wv1;
                bilinear_weight_pairs(nxp - fx, nyp - fy, wv0, wv1);
                int s1, s2;
                lane_mismatch<CA>(V, wv0, wv1, Ixp, Iyp, neg_c1, neg_c2, s1, s2);
                float b1, b2;
                wave_sum2_float<MUL>(s1, s2, b1, b2);
                const float dx = (A12 * b2 - A22 * b1) * Dds;
                const float dy = (A12 * b1 - A11 * b2) * Dds;
                nxp += dx;
                nyp += dy;
                stepped = true;
                more = false;
                // |dx|^2 + |dy|^2 <= eps^2 in double, as the reference; only a step that is small in float
                // can pass, so the double arithmetic is skipped for all the others
                if (uniform(fmaxf(fabsf(dx), fabsf(dy)) <= prm.eps_pre) &&
                    uniform((double)dx * (double)dx + (double)dy * (double)dy <= prm.eps_sq))
                    break;
                // fabs((double)x) < 0.01  <=>  |x| <= 0.01f for a float x: 0.01f is the largest float below 0.01
                if (j > 0 && uniform(fabsf(dx + pdx) <= 0.01f && fabsf(dy + pdy) <= 0.01f)) {
                    outx = (nxp + half) - dx * 0.5f;
                    outy = (nyp + half) - dy * 0.5f;
                    out_set = true;
                    break;
                }
                pdx = dx;
                pdy = dy;
                if (++j >= prm.max_count)
                    break;
                fx = floorf(nxp);
                fy = floorf(nyp);
                inx = uniform_int_of(fx);
                iny = uniform_int_of(fy);
                if (inx < -WIN || inx >= lw || iny < -WIN || iny >= lh) {
                    if (level == 0)
                        st = 0;
                    break;
                }
                more = true;
                if (!prm.cell_cache || inx != cx || iny != cy)
                    break;  // another cell: load and pair its rows
            }
        }
        // the reference keeps nextPt = guess + half up to date inside the loop; the same float operations
        // in the same order, once, after it
        if (stepped && !out_set) {
            outx = nxp + half;
            outy = nyp + half;
        }

        // ---- 3. level-0 residual (err output of calcOpticalFlowPyrLK) ----
        if (st && level == 0) {
            const float qx = outx - half, qy = outy - half;
            const int iqx = uniform_int_of(floorf(qx)), iqy = uniform_int_of(floorf(qy));
            if (iqx < -WIN || iqx >= lw || iqy < -WIN || iqy >= lh) {
                st = 0;
                continue;
            }
            // without WANT_ERR no caller of this launch reads err: only the bounds test above affects its outputs
            if constexpr (WANT_ERR) {
                if (uniform(err == nullptr))
                    continue;  // this job's caller does not read it
                if (!have_tile || iqx < ox || iqx > ox + 2 * JR || iqy < oy || iqy > oy + 2 * JR) {
                    ox = iqx - JR;
                    oy = iqy - JR;
                    wave_lds_sync();
                    tj_off = (int)(TJ - lds) + uniform(stage_tile<CS, TS>(TJ, J, pitch, ox, oy, lane));
                    wave_lds_sync();
                    have_tile = true;
                }
                int w00, w01, w10, w11;
                bilinear_weights(qx - (float)iqx, qy - (float)iqy, w00, w01, w10, w11);
                int Iv0[npairs(CA)];
                if constexpr (PARK_IVP) {
                    const int *park = reinterpret_cast<const int *>(lds + PARK) + lane;
#pragma unroll
                    for (int k = 0; k < npairs(CA); k++)
                        Iv0[k] = park[64 * k];
                } else {
#pragma unroll
                    for (int k = 0; k < npairs(CA); k++)
                        Iv0[k] = Ivp[k];
                }
                int s1 = lane_abs_residual<CA, CS>(lds, lane_off + (tj_off + (iqy - oy) * Tile<CS, TS>::ROW + (iqx - ox) * CS),
                                              (w00 & 0xffff) | (w10 << 16), (w01 & 0xffff) | (w11 << 16), Iv0);
                if (!active)
                    s1 = 0;
                const long long sabs = (long long)wave_sum_exact(s1) * MUL;  // < 2^24, the factor included
                errv = (float)sabs / (float)(32 * WIN * C * WIN);
            }
        }
    }
