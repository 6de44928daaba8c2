// cec_combo.inc -- the vocabulary every op states its GF(2^8) combination in.
// Included by cec_runtime.hip ahead of the launch internals and the ops; not a separate TU.
//
//   Code     a view of the coding matrix: at(row, col)
//   Streams  the byte streams of one launch: add(base) hands out the next slot
//   Combo    one linear combination: in(slot) returns the input's index, out(slot, mode)
//            the output whose coef[input index] the op sets; build_patterns makes the
//            kernels' Patterns of it, kPatL outputs per launch
//   fold / multiply_combo   the combinations more than one op runs
//   Loss     what a recovery mask loses: lost lids, participating parities, surviving
//            data lids, and the inverse that rebuilds the lost from the parities' residuals

// The (k + m) x k coding matrix, row-major (MATRIX(x, y) of memcached.h:52).  A view: the
// caller's array for the length of a call, or the copy a session owns.
struct Code {
    int k = 0, m = 0;
    const int *matrix = nullptr;
    int at(int row, int col) const { return matrix[row * k + col]; }
    // A session's view over its own copy of the caller's matrix.
    static Code owned(std::vector<int> &store, int k, int m, const int *matrix) {
        store.assign(matrix, matrix + (k + m) * k);
        return {k, m, store.data()};
    }
};

// The byte streams of one launch (the kernels' base[]).  Slots are handed out in the order
// an op names its streams and a combination refers to a stream by the slot add returned,
// so the two cannot drift apart.
struct Streams {
    uint8_t *base[kMaxStreams] = {};
    int n = 0;
    bool refused = false;  // a slot past the last was asked for: launch_combine refuses
    // The next slot, holding `b`.  A NULL b still takes its slot, which stays empty (a lost
    // parity, an output the call did not ask for): no pattern of the launch may name it.
    int add(const void *b) {
        if (n == kMaxStreams) {
            refused = true;
            (void)fail(CEC_EINVAL, "internal: an op names more than %d byte streams; not launched", kMaxStreams);
            return 0;
        }
        base[n] = static_cast<uint8_t *>(const_cast<void *>(b));
        return n++;
    }
};

// Logical pattern with arbitrarily many outputs, before splitting.
struct Combo {
    int n_in = 0;
    uint8_t in_stream[kPatN] = {};
    uint8_t in_src[kPatN] = {};
    struct Out {
        uint8_t stream, src, mode;
        int coef[kPatN];
    };
    // An output that overwrites one of the inputs (the diff-update's install, the fused
    // finish's R') is last: past kPatL outputs the launches run in order (build_patterns).
    std::vector<Out> outs;

    // One more input: stream `slot`, addressed by the tile's src_off (`by_src`) or its off.
    // Returns the input's index into every output's coef[].  Past kPatN nothing is stored
    // and n_in still counts, so build_patterns refuses the combination.
    int in(int slot, bool by_src = false) {
        if (n_in >= kPatN) {
            ++n_in;
            (void)fail(CEC_EINVAL, "internal: a combination of more than %d inputs; not launched", kPatN);
            return 0;
        }
        in_stream[n_in] = static_cast<uint8_t>(slot);
        in_src[n_in] = by_src;
        return n_in++;
    }
    // One more output, all coefficients 0: stream `slot`, written (kModeWrite) or XORed into
    // (kModeXor).  The reference holds until the next out().
    Out &out(int slot, int mode, bool by_src = false) {
        outs.push_back(Out{static_cast<uint8_t>(slot), by_src, static_cast<uint8_t>(mode), {}});
        return outs.back();
    }
};

// dst = c * src, or dst ^= c * src (`add`): the region multiply.
static Combo multiply_combo(int c, bool add, int src_slot, int dst_slot) {
    Combo cb;
    cb.out(dst_slot, add ? kModeXor : kModeWrite).coef[cb.in(src_slot)] = c;
    return cb;
}

// The fold of shipped diffs into a parity's bytes (process_rep_command, memcached.c:7739-7767;
// into a recovery residual, recovery.c:123): target ^= M[self][j] * diff, the diffs addressed
// by src_off.  One pattern per source shard j, the pattern index; with `only`, the one
// pattern of that shard.  Slots 0 and 1: the narrow 1 x 1 kernels serve it.
struct Fold {
    Streams st;
    std::vector<Combo> combos;
};
static Fold fold(const Code &code, int lid_self, const uint8_t *diffs, uint8_t *target, int only = -1) {
    Fold f;
    const int d = f.st.add(diffs), t = f.st.add(target);
    for (int j = only < 0 ? 0 : only; j < (only < 0 ? code.k : only + 1); ++j) {
        Combo c;
        c.out(t, kModeXor).coef[c.in(d, true)] = code.at(lid_self, j);
        f.combos.push_back(c);
    }
    return f;
}

static int mask_ok(int k, int m, uint32_t mask) {
    if (k + m < 32 && (mask >> (k + m)) != 0) return 0;
    return __builtin_popcount(mask) == k;
}

// What a recovery mask loses (complete_recovery_bottom_half, memcached.c:7847-7907): the
// data lids outside the mask, as many participating parities, the data lids inside it, all
// ascending, and inv = (M[pars][lost])^-1: lost[x] = sum_r at(x, r) * residual of pars[r].
struct Loss {
    int n = 0;       // lost data lids = participating parities
    int n_surv = 0;  // = k - n
    int lost[CEC_MAX_K], pars[CEC_MAX_M], surv[CEC_MAX_K];
    int inv[CEC_MAX_M * CEC_MAX_M];
    int at(int x, int r) const { return inv[x * n + r]; }
    int index_of_parity(int lid) const {
        for (int r = 0; r < n; ++r)
            if (pars[r] == lid) return r;
        return -1;
    }
    // `invert` = false leaves inv alone (the pool's single losses: one coefficient's inverse).
    static int of(const Code &code, uint32_t mask, const char *op, Loss *out, bool invert = true) {
        if (!mask_ok(code.k, code.m, mask)) return fail(CEC_EINVAL, "%s: mask 0x%x is not a recovery mask", op, mask);
        Loss &l = *out;
        l.n = l.n_surv = 0;
        int r = 0;
        for (int j = 0; j < code.k; ++j) {
            if (mask & (1u << j)) l.surv[l.n_surv++] = j;
            else l.lost[l.n++] = j;
        }
        for (int p = code.k; p < code.k + code.m; ++p)
            if (mask & (1u << p)) l.pars[r++] = p;  // (k lids in the mask: r == n)
        if (!invert || l.n == 0) return CEC_OK;
        int tmp[CEC_MAX_M * CEC_MAX_M];
        for (int x = 0; x < l.n; ++x)
            for (int c = 0; c < l.n; ++c) tmp[x * l.n + c] = code.at(l.pars[x], l.lost[c]);
        if (invert_matrix(tmp, l.inv, l.n))
            return fail(CEC_ESINGULAR, "%s: singular submatrix for mask 0x%x", op, mask);
        return CEC_OK;
    }
};
