// fold_popcount_body.inc -- the one loop of the popcount fold, as text:
// included inside the body of k_fold_sliced_direct (pir_fold_sliced.hip, one
// key) and of k_fold_grouped<KP> (pir_fold_grouped.hip), behind each kernel's
// own prologue; text for the reason given in fold_mfma_body.inc.  Thread n of
// the workgroup's 256 owns bit row `row` = 256 * column + n; per super-group of
// [s0, s1) it reads the row's 8 words once and XORs (word & selection word)
// into each key's accumulator: one v_bitop3 per word and key, the selection
// words wave-uniform (scalar loads).  A thread whose row does not exist
// (row >= nrows) folds nothing.  Answer bit n of key j is the parity of
// popcount(acc[j]): one ballot per key, two answer words per wave.
//
// In scope at the #include, from the kernel:
//   KP                keys folded together; FOLD_ONE_KEY defined: KP is 1 and
//                     the kernel was written for one key (no loop over keys);
//   n, col            the thread's index and the workgroup's column;
//   s0, s1, nrows     the run of super-groups; bit rows of a super-group;
//   wlim, FOLD_SEL(j, i)  key j's selection row has wlim words and
//                     FOLD_SEL(j, i) is its word i, word 8 S + q for super-group
//                     S; words at or past wlim select nothing;
//   FOLD_AT(S)        -> const uint4*: the two uint4 of bit row `row` in
//                     super-group S;
//   FOLD_EMIT_BEGIN   statements once behind the loop, what FOLD_EMIT needs;
//   FOLD_EMIT(j, m)   statement: key j's ballot m -- lane 0 of a wave writes
//                     its low word, lane 1 its high word.
    uint32_t acc[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) acc[j] = 0;
    auto fold = [&](uint64_t S, const uint4& a, const uint4& b) __attribute__((always_inline)) {
        const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (8 * S + 8 <= wlim) {                               // uniform
#pragma unroll
            for (int j = 0; j < KP; ++j)
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[j] = xam(acc[j], x[q], FOLD_SEL(j, 8 * S + q));
        } else {                                               // the key rows end inside this super-group
#pragma unroll
            for (int j = 0; j < KP; ++j)
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (8 * S + q < wlim) acc[j] = xam(acc[j], x[q], FOLD_SEL(j, 8 * S + q));
        }
    };
    const uint64_t row = (uint64_t)col * 256 + n;
    auto at = [&](uint64_t S) { return FOLD_AT(S); };
    if (row < nrows) {
        uint64_t S = s0;
        for (; S + 1 < s1; S += 2) {
            const uint4 a0 = at(S)[0], b0 = at(S)[1];
            const uint4 a1 = at(S + 1)[0], b1 = at(S + 1)[1];
            fold(S, a0, b0);
            fold(S + 1, a1, b1);
        }
        if (S < s1) fold(S, at(S)[0], at(S)[1]);
    }
    FOLD_EMIT_BEGIN
    auto answer = [&](int j) __attribute__((always_inline)) {
        const uint64_t m = __builtin_amdgcn_ballot_w64((__builtin_popcount(acc[j]) & 1) != 0);
        FOLD_EMIT(j, m)
    };
#ifdef FOLD_ONE_KEY
    answer(0);                                                 // not a loop of one: that moves the kernel's store address
#else
#pragma unroll
    for (int j = 0; j < KP; ++j) answer(j);
#endif
#undef FOLD_ONE_KEY
#undef FOLD_SEL
#undef FOLD_AT
#undef FOLD_EMIT_BEGIN
#undef FOLD_EMIT
