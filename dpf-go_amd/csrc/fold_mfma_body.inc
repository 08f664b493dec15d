// fold_mfma_body.inc -- the one loop of the matrix-core fold, as text: included
// as the body of k_fold_mfma (pir_fold_sliced.hip: the layout, the operands and
// why the fp32 counts are exact) and of k_fold_grouped_mfma
// (pir_fold_grouped_mfma.hip).  It is the wave decode, the staging of selection
// rows through LDS, the double-buffered block loop, the FP4 operand expansion,
// the MFMA nest and the ballot epilogue; what differs between the kernels is
// five macros that the kernel defines before the #include (undefined again at
// the end of this file).  Text and not a function template with callables:
// the kernels' tile shapes were picked by what does not spill, and only this
// form compiles every instantiation of both kernels to the instructions it had
// with a loop of its own (tools/fold_isa_compare.py, profiles/fold_shared_body/).
//
// In scope at the #include: MT, NT, SG, CG (the tile shape of dpfh::kFoldTiles),
// FULL (every bit tile exists), ntiles (bit tiles of a record) and wlim.
//   FOLD_UNIT    statements behind the wave decode (l, h, r, w, cw).  Defines
//                col0, the first column of the workgroup's column group (wave
//                wv takes bit slice wv % NS of column col0 + wv / NS), and the
//                selection rows: row j < nrows starts at sel + j * stride and
//                has wlim words, word 8 * S + q for super-group S; rows from
//                nrows on and words at or past wlim are staged as zeros and
//                not read.  Defines NTDB (nontemporal DB loads) unless it is a
//                template parameter.
//   FOLD_RUN     statements behind tile0 and nt; with FOLD_UNIT defines the
//                workgroup's run of super-groups [s0, s1), s0 < s1 (it may
//                return for an empty run).
//   FOLD_DB_AT(S, j)  -> const uint4*: this lane's piece (row r, half h) of bit
//                tile tile0 + j of super-group S.  Used for tiles < ntiles and
//                S in [s0, s1) only (loads past the run are clamped inside it
//                and never folded).
//   FOLD_EMIT_BEGIN   statements once behind the block loop: what FOLD_EMIT
//                needs, read there so that it is not held across the loop.
//   FOLD_EMIT(m, j, out)  statement: `out` is the answer word of key row
//                32 * m + l and bit tile tile0 + j in lanes l < 32; the guards
//                (l < 32, j < nt, the kernel's own) are the macro's.
    constexpr int NS = 8 / NT;                                 // bit slices of a column
    constexpr int NW = NS * CG;
    constexpr bool SC = NT < MT;                               // the selection side takes the cheap expansion
    constexpr int kRows = 32 * MT;
    constexpr int kRow = SG * 8 + 4;                           // words per staged row (+4: conflict-free b128 reads)
    constexpr int kPieces = kRows * (SG * 2);                  // uint4 pieces per staged block
    constexpr int kPer = (kPieces + 64 * NW - 1) / (64 * NW);  // per thread
    __shared__ __attribute__((aligned(16))) uint32_t s_sel[kRows * kRow];
    const uint32_t l = threadIdx.x & 63, h = l >> 5, r = l & 31;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w = wv % NS, cw = wv / NS;                   // bit slice, column of the group
    FOLD_UNIT
    const uint64_t col = col0 + cw;
    const uint64_t tile0 = 8 * col + w * NT;                    // this wave's first bit tile
    const uint32_t nt =                                         // how many of its NT tiles the record has
        FULL ? (uint32_t)NT
             : __builtin_amdgcn_readfirstlane(tile0 >= ntiles               ? 0u
                                              : ntiles - tile0 < (uint64_t)NT ? (uint32_t)(ntiles - tile0)
                                                                              : (uint32_t)NT);
    FOLD_RUN
    auto load_sel = [&](uint64_t sb, uint4 (&v)[kPer]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const uint32_t p = threadIdx.x + (uint32_t)i * 64 * NW;
            const uint32_t row = p / (2 * SG), q = p % (2 * SG);
            const uint64_t word = sb * 8 + 4 * q;
            const bool ok = p < (uint32_t)kPieces && row < nrows && word + 4 <= wlim;
            const uint4 x = *reinterpret_cast<const uint4*>(sel + (ok ? (uint64_t)row * stride + word : 0));
            v[i] = ok ? x : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_sel = [&](const uint4 (&v)[kPer]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const uint32_t p = threadIdx.x + (uint32_t)i * 64 * NW;
            if (p < (uint32_t)kPieces) *reinterpret_cast<uint4*>(&s_sel[(p / (2 * SG)) * kRow + 4 * (p % (2 * SG))]) = v[i];
        }
    };
    // DB pieces of a whole block (clamped past the run; never folded).  A
    // tile the record does not have is not loaded: zeros.
    auto load_db = [&](uint64_t sb, uint4 (&B)[SG][NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int sl = 0; sl < SG; ++sl) {
            const uint64_t S = sb + sl < s1 ? sb + sl : s1 - 1;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                B[sl][j] = make_uint4(0, 0, 0, 0);
                if ((uint32_t)j < nt) B[sl][j] = fold_ld<NTDB>(FOLD_DB_AT(S, j));
            }
        }
    };
    fold_v16f acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][j][e] = 0.0f;
    // One super-group: 4 K-blocks of 64 records x MT x NT MFMAs.
    auto fold_sg = [&](int sl, const uint4 (&B)[NT]) __attribute__((always_inline)) {
        uint4 A[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            A[m] = *reinterpret_cast<const uint4*>(&s_sel[(32 * m + r) * kRow + 8 * sl + 4 * h]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            fold_v8i bo[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) bo[j] = fp4_db<SC>(u4w(B[j], t));
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const fold_v8i ao = fp4_sel<SC>(u4w(A[m], t));
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[m][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ao, bo[j], acc[m][j], kFoldFp4, kFoldFp4,
                                                                               0, kE8M0One, 0, kE8M0One);
            }
        }
    };
    uint4 sv[kPer];
    uint4 BA[SG][NT], BB[SG][NT];
    load_sel(s0, sv);
    load_db(s0, BA);
    // One staged block: its selection rows to LDS, the next block's loads
    // issued, then its super-groups folded.
    auto block = [&](uint64_t sb, const uint4 (&Bc)[SG][NT], uint4 (&Bn)[SG][NT]) __attribute__((always_inline)) {
        lds_barrier();                                          // previous block's operand reads are done
        store_sel(sv);
        lds_barrier();
        const uint64_t nb = sb + SG < s1 ? sb + SG : sb;        // next block (clamped)
        load_sel(nb, sv);
        load_db(nb, Bn);
        const uint64_t n = s1 - sb;
#pragma unroll
        for (int sl = 0; sl < SG; ++sl)
            if ((uint64_t)sl < n && nt != 0) fold_sg(sl, Bc[sl]);
    };
    uint64_t sb = s0;
    for (; sb + SG < s1; sb += 2 * SG) {
        block(sb, BA, BB);
        block(sb + SG, BB, BA);
    }
    if (sb < s1) block(sb, BA, BB);
    FOLD_EMIT_BEGIN
    // Parities -> answer words (C/D layout: lane = column n, register e = rows
    // (e&3) + 8(e>>2) + 4h): one ballot per accumulator register.
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            uint32_t out = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t p = ((uint32_t)acc[m][j][e]) & 1u;
                const uint64_t b = __builtin_amdgcn_ballot_w64(p != 0);
                const uint32_t row0 = (e & 3) + 8 * (e >> 2);
                out = l == row0 ? (uint32_t)b : out;
                out = l == row0 + 4 ? (uint32_t)(b >> 32) : out;
            }
            FOLD_EMIT(m, j, out)
        }
#undef FOLD_UNIT
#undef FOLD_RUN
#undef FOLD_DB_AT
#undef FOLD_EMIT_BEGIN
#undef FOLD_EMIT
