// Validation, kernel choice and dispatch behind sad_mlp_chain_f32 / sad_mlp_chain_multi_f32 (SPEC.md §6): the tiled
// kernel (mlp_chain.hip), the register-resident chain (mlp_reg.hip), the layer-streamed chain (mlp_layer.hip), the
// cooperative register-resident chain (mlp_coop.hip) and the vector-ALU kernel.
// No reference source exists (/root/reference/README.md:1-2 is the whole upstream repository).
#include "mlp_chain.h"

using namespace sad::chain;

namespace {
// the kernel a prepared chain runs on: VALU_DONE = the VALU kernel was launched by its preparer (nothing left to do)
enum Kind { VALU_DONE, TILED, REG, COOP, ROWS, LAYERED };
struct Prepared {
    Kind kind;
    MlpParams p;           // TILED: the tiled kernel (mlp_chain.hip), with lds, nblocks, W, RW, CW
    size_t lds;
    long long nblocks;
    int W, RW, CW;
    sad::RegChain rc;      // REG (geometry 2): register-resident chain kernel (mlp_reg.hip), COOP (geometry 4): its cooperative variant (mlp_coop.hip)
    int reg_shape;
    long long reg_tiles;   // upper bound of the tile count
    sad::ScanJob scan;     // row-packing scan this chain needs before its kernel
    bool prescanned;       // ... unless the caller already ran sad_mlp_rowscan on the workspace (or the chain has no row map)
    sad::RowsJob rj;       // ROWS (geometry 5): row-streaming plain layer (mlp_rows.hip)
    sad::LayerJob lj[MAXL];    // LAYERED (geometry 3): layer-streamed chain (mlp_layer.hip); lj[0..nl) are its launches
    int nl;
    long long layer_items[MAXL];
};
// what the validation of an argument block hands to the preparer of the kernel that was asked for
struct Chain {
    const sad_mlp_args *a;
    Geometry g;
    MlpParams p;                                // the parameters every kernel shares (p.grouped, p.cout_last = the caller's output channels, ..)
    int geom_wg, flex_code, dyn_code, dedup_f;  // the digits of the geometry code, the assumed ratio of padded to surviving rows
};
bool all_relu(const sad_mlp_args *a) { return (a->relu_mask & ((1 << a->L) - 1)) == (1 << a->L) - 1; }
}  // namespace

// Validation of one argument block and the parameters every kernel shares.
static int chain_args(const sad_mlp_args *a, Chain &c) {
    SAD_REQUIRE(a, "sad_mlp_chain_f32: NULL args");
    SAD_REQUIRE(a->struct_size == sizeof(sad_mlp_args), "sad_mlp_chain_f32: struct_size=%zu, this library's sad_mlp_args has %zu bytes "
                "(caller built against another sad_amd.h; ABI version %d)", a->struct_size, sizeof(sad_mlp_args), SAD_ABI_VERSION);
    if (int e = check_dims("sad_mlp_chain_f32", a->L, a->dims)) return e;
    const bool grouped = a->idx != nullptr;
    SAD_REQUIRE(a->packed && a->out, "sad_mlp_chain_f32: NULL packed/out");
    SAD_REQUIRE(a->B >= 1 && a->M >= 1 && a->C >= 0, "sad_mlp_chain_f32: bad B/M/C");
    SAD_REQUIRE(a->C == 0 || a->feat, "sad_mlp_chain_f32: C=%d but feat is NULL", a->C);
    SAD_REQUIRE(a->C == 0 || a->ld_feat >= a->C, "sad_mlp_chain_f32: ld_feat=%d < C=%d", a->ld_feat, a->C);
    if (grouped) {
        SAD_REQUIRE(a->xyz && a->new_xyz, "sad_mlp_chain_f32: grouped mode needs xyz and new_xyz");
        SAD_REQUIRE(a->N >= 1 && a->S >= 1 && a->S <= 64, "sad_mlp_chain_f32: need N>=1, 1<=S<=64 (S=%d)", a->S);
        if (a->c_out)       // a chain packed zero-padded onto wider dims (sad_mlp_padded_dims): fewer feature channels than dims[0] - 3
            SAD_REQUIRE(a->C + 3 <= a->dims[0] && a->c_out >= 1 && a->c_out <= a->dims[a->L],
                        "sad_mlp_chain_f32: zero-padded chain needs C+3=%d <= dims[0]=%d and 1 <= c_out=%d <= dims[L]=%d", a->C + 3, a->dims[0], a->c_out, a->dims[a->L]);
        else
            SAD_REQUIRE(a->dims[0] == a->C + 3, "sad_mlp_chain_f32: dims[0]=%d != C+3=%d", a->dims[0], a->C + 3);
        SAD_REQUIRE((long long)a->B * a->N < (1LL << 31), "sad_mlp_chain_f32: B*N too large");
        SAD_REQUIRE((long long)a->B * a->M * a->S < (1LL << 31), "sad_mlp_chain_f32: B*M*S too large (row numbers are 32-bit)");
        // straddling groups are merged with an unsigned atomic max into a zero-initialised buffer:
        // only valid for non-negative outputs, i.e. a ReLU after every layer (SPEC.md §6 grouped chains)
        SAD_REQUIRE(all_relu(a), "sad_mlp_chain_f32: grouped chains need a ReLU after every layer (relu_mask=0x%x, L=%d)", a->relu_mask, a->L);
    } else {
        SAD_REQUIRE(a->S == 1, "sad_mlp_chain_f32: plain mode needs S == 1");
        SAD_REQUIRE(a->c_out == 0, "sad_mlp_chain_f32: c_out (zero-padded chain) is a grouped-mode field");
        SAD_REQUIRE(a->C >= 1 && a->dims[0] == a->C, "sad_mlp_chain_f32: dims[0]=%d != C=%d", a->dims[0], a->C);
        SAD_REQUIRE((long long)a->B * a->M < (1LL << 31), "sad_mlp_chain_f32: too many rows");
    }
    const int cout = a->c_out ? a->c_out : a->dims[a->L];
    SAD_REQUIRE(a->ld_out >= a->col_off + cout && a->col_off >= 0, "sad_mlp_chain_f32: ld_out=%d too small for col_off=%d + C_out=%d", a->ld_out, a->col_off, cout);

    c.a = a;
    c.g = geometry(a->L, a->dims, grouped);
    MlpParams &p = c.p;
    p = MlpParams{};
    p.xyz = a->xyz; p.new_xyz = a->new_xyz; p.idx = a->idx; p.cnt = a->cnt; p.feat = a->feat; p.packed = a->packed;
    p.out = a->out; p.ld_feat = a->ld_feat; p.N = a->N; p.M = a->M; p.S = a->S; p.C = a->C;
    p.grouped = grouped; p.L = a->L; p.relu_mask = a->relu_mask; p.ld_out = a->ld_out;
    p.col_off = a->col_off; p.cout_last = cout;
    int sp_shift = 0;
    while ((1 << sp_shift) < a->S) ++sp_shift;
    p.sp_shift = sp_shift;
    p.total_rows = (long long)a->B * a->M << sp_shift;   // plain mode: rows; VALU kernel: padded rows
    p.total_groups = (long long)a->B * a->M;
    // (the mlp_force knob of tests / sweeps wins over the per-call field)
    const int geom_all = sad::get_option(sad::OPT_MLP_FORCE) ? sad::get_option(sad::OPT_MLP_FORCE) : a->geometry;
    c.flex_code = (geom_all / 100000) % 10;          // bit 0 = flexible item distribution, bit 1 = two output tiles per wave (both need RW == 1)
    c.dyn_code = (geom_all / 10000) % 10;            // 0 = heuristic, 1 = global packing, 2 = per-workgroup packing
    const int fcode = (geom_all / 1000) % 10;        // 0 = default
    c.geom_wg = geom_all % 1000;
    c.dedup_f = sad::get_option(sad::OPT_MLP_DEDUP_F) > 0 ? sad::get_option(sad::OPT_MLP_DEDUP_F) : 8;
    if (fcode >= 1 && fcode <= 7) c.dedup_f = 1 << fcode;
    if (sad::get_option(sad::OPT_MLP_NODEDUP)) c.dedup_f = 1;
    for (int l = 0; l < a->L; ++l) { p.kp[l] = c.g.kp[l]; p.np[l] = c.g.np[l]; p.off[l] = c.g.off[l]; }
    p.vec_out = (a->ld_out % 4 == 0 && a->col_off % 4 == 0 && ((uintptr_t)a->out % 16 == 0)) ? 1 : 0;
    // feature staging: 16-B chunks when rows are 16-B aligned
    if (a->C >= 4 && a->C % 4 == 0 && a->ld_feat % 4 == 0 && ((uintptr_t)a->feat % 16 == 0)) {
        p.cpr = a->C / 4;
        int cs = 0;
        while ((1 << cs) < p.cpr && cs < 6) ++cs;
        p.cshift = cs;
    }
    if (a->c_out && c.geom_wg != 2 && c.geom_wg != 4)
        return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: a zero-padded chain (c_out != 0) runs on geometries 2 / 4 only (geometry %d asked)", c.geom_wg);
    return SAD_OK;
}

// Row-packing scan of a chain whose kernel reads a row map of 32-row tiles, launched by the caller (the chains of a merged dispatch share its two launches)
static int chain_scan(const Chain &c, Prepared &q) {
    const sad_mlp_args *a = c.a;
    SAD_REQUIRE(c.p.total_groups < (1LL << 30), "sad_mlp_chain_f32: too many groups");
    q.scan = sad::make_scan_job(a->cnt, (int)c.p.total_groups, a->S, 32, (int *)a->workspace, sad::get_option(sad::OPT_MLP_NODEDUP), a->idx, a->N, a->M);
    sad::scan_zero_fill(q.scan, a->out, a->ld_out, a->col_off, c.p.cout_last);
    return SAD_OK;
}

// Geometries 2 / 4: register-resident chain (one wave per 32-row tile, no LDS round trips, no barriers) and its cooperative variant.
static int prepare_reg(const Chain &c, Prepared &q) {
    const sad_mlp_args *a = c.a;
    const Geometry &g = c.g;
    const int shape = c.p.grouped ? sad::reg_shape_id(a->L, g.kp, g.np) : -1;
    if (c.geom_wg == 4 && (shape < 0 || !sad::coop_shape(shape) || g.stream_off < 0 || c.p.cpr <= 0))
        return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry 4 (cooperative register-resident chain) is compiled for the SA2 / SA3 shapes");
    const bool feat_ok = a->C == 0 || a->C == 1 || c.p.cpr > 0;
    if (shape < 0 || !all_relu(a) || !feat_ok || !a->cnt || !a->workspace)
        return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry 2 (register-resident chain) needs a compiled 3-layer shape, "
                                           "cnt + workspace and 16-byte feature rows");
    SAD_REQUIRE((uintptr_t)a->workspace % 16 == 0, "sad_mlp_chain_f32: workspace must be 16-byte aligned");
    if (int e = chain_scan(c, q)) return e;
    sad::RegChain &rc = q.rc;
    rc.xyz = a->xyz; rc.new_xyz = a->new_xyz; rc.feat = a->feat; rc.packed = a->packed; rc.out = a->out;
    rc.rowtab = q.scan.tab; rc.row_src = q.scan.row_src; rc.row_gid = q.scan.row_gid;
    for (int l = 0; l < 3; ++l) { rc.off[l] = g.off[l]; rc.np[l] = g.np[l]; }
    rc.stream_off = g.stream_off;
    rc.ld_feat = a->ld_feat; rc.C = a->C; rc.cpr = c.p.cpr;
    rc.ld_out = a->ld_out; rc.col_off = a->col_off; rc.cout_last = c.p.cout_last; rc.vec_out = c.p.vec_out;
    q.kind = c.geom_wg == 4 ? COOP : REG;
    q.reg_shape = shape;
    q.reg_tiles = (c.p.total_groups * a->S + 31) / 32;
    return SAD_OK;
}

// Geometry 5: row-streaming plain layer (one layer, every input row read once per 128 output channels).
static int prepare_rows(const Chain &c, Prepared &q) {
    const sad_mlp_args *a = c.a;
    const Geometry &g = c.g;
    if (c.p.grouped || a->L != 1 || c.p.cpr <= 0 || a->C % 8 != 0 || g.kp[0] != a->C)
        return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry 5 (row-streaming layer) takes one plain layer with C %% 8 == 0 "
                                           "and 16-byte aligned rows");
    sad::RowsJob &j = q.rj;
    j = sad::RowsJob{};
    j.x = a->feat; j.ldx = a->ld_feat; j.rows = c.p.total_rows;
    j.packed = a->packed; j.off = g.off[0]; j.np = g.np[0]; j.kg = g.kp[0] / 8; j.ct = g.np[0] / 32; j.cout = c.p.cout_last;
    j.relu = a->relu_mask & 1;
    j.out = a->out; j.ld_out = a->ld_out; j.col_off = a->col_off; j.vec_out = c.p.vec_out;
    q.kind = ROWS;
    return SAD_OK;
}

// Geometry 3: layer-streamed chain (one launch per layer, activations between layers in the two ping-pong buffers of `scratch`).
//   plain rows: every layer is a row-major GEMM launch (bias + optional ReLU); the last one writes the caller's output slice, whole
//               128-channel blocks at a time, so C_out must be its own padded width
//   grouped:    the rows are those of the row map; layer 0 gathers them, the last layer pools them into the caller's output slice
static int prepare_layered(const Chain &c, Prepared &q) {
    const sad_mlp_args *a = c.a;
    const Geometry &g = c.g;
    const MlpParams &p = c.p;
    const bool grouped = c.p.grouped;
    const int L = a->L;
    bool ok = p.cpr > 0;
    for (int l = 0; l < L; ++l) ok = ok && g.np[l] % 128 == 0 && (l == 0 || g.kp[l] == g.np[l - 1]);
    if (grouped) {
        ok = ok && a->cnt && a->workspace && a->scratch && all_relu(a) && a->scratch_bytes >= sad_mlp_scratch_bytes(a->B, a->M, a->S, L, a->dims);
        if (!ok)
            return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry 3 (layer-streamed chain) needs cnt + workspace + scratch, "
                                               "16-byte feature rows and layer widths that are multiples of 128");
        SAD_REQUIRE((uintptr_t)a->workspace % 16 == 0 && (uintptr_t)a->scratch % 16 == 0, "sad_mlp_chain_f32: workspace / scratch must be 16-byte aligned");
        if (int e = chain_scan(c, q)) return e;
    } else {
        ok = ok && a->C % 8 == 0 && p.vec_out && g.np[L - 1] == p.cout_last && (L == 1 || (a->scratch && a->scratch_bytes >= sad_mlp_scratch_bytes(a->B, a->M, 1, L, a->dims)));
        if (!ok)
            return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry 3 (layer-streamed chain) on plain rows needs 16-byte rows, "
                                               "C %% 8 == 0, layer widths that are multiples of 128 and, for L > 1, scratch");
        SAD_REQUIRE(L == 1 || (uintptr_t)a->scratch % 16 == 0, "sad_mlp_chain_f32: scratch must be 16-byte aligned");
        q.prescanned = true;     // no row map
    }
    const long long in_rows = grouped ? (long long)a->B * a->N : p.total_rows;                   // feature rows layer 0 may read
    const long long rows_max = ((grouped ? p.total_groups * a->S : p.total_rows) + 31) / 32 * 32;    // rows of a hidden activation matrix
    // mlp_layer.hip forms the byte offset of an input row as a 32-bit product (row * ld * 4): the first layer's feature rows and every
    // hidden activation matrix (rows_max x np[l]) must stay below 4 GiB
    bool fit = in_rows * a->ld_feat * 4 < (1LL << 32);
    for (int l = 0; l + 1 < L; ++l) fit = fit && rows_max * g.np[l] * 4 < (1LL << 32);
    if (!fit && grouped)
        return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry 3 (layer-streamed chain): rows x row stride x 4 must stay below 4 GiB "
                                           "(B*N = %lld feature rows, %lld grouped rows); split the call or use the tiled kernel", in_rows, rows_max);
    if (!fit)
        return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry 3 (layer-streamed chain): rows x row stride x 4 must stay below 4 GiB "
                                           "(%lld rows); split the call or use the tiled kernel", p.total_rows);
    int wa = 0;                                  // width of the first ping-pong buffer: the widest output of the even hidden layers
    for (int l = 0; l + 1 < L; l += 2) wa = g.np[l] > wa ? g.np[l] : wa;
    float *ha = L > 1 || grouped ? (float *)((char *)a->scratch + 64) : nullptr;
    float *hb = ha ? ha + rows_max * wa : nullptr;
    q.nl = L;
    for (int l = 0; l < L; ++l) {
        sad::LayerJob &j = q.lj[l];
        j = sad::LayerJob{};
        j.packed = a->packed; j.off = g.off[l]; j.np = g.np[l]; j.kg = g.kp[l] / 8; j.nog = g.np[l] / 128;
        j.relu = (a->relu_mask >> l) & 1;
        if (l == 0) { j.x = a->feat; j.ldx = a->ld_feat; }
        else { j.x = ((l - 1) & 1) ? hb : ha; j.ldx = g.np[l - 1]; }
        if (l + 1 < L) { j.y = (l & 1) ? hb : ha; j.ldy = g.np[l]; }
        if (grouped) {
            j.rowtab = q.scan.tab; j.row_src = q.scan.row_src; j.row_gid = q.scan.row_gid;
            j.last = l == L - 1;
            if (l == 0) { j.gather = 1; j.cpr = p.cpr; j.xyz = a->xyz; j.new_xyz = a->new_xyz; }
            if (j.last) { j.out = a->out; j.ld_out = a->ld_out; j.col_off = a->col_off; j.cout_last = c.p.cout_last; }
        } else {
            j.rows = (int)p.total_rows;
            if (l == L - 1) { j.y = a->out + a->col_off; j.ldy = a->ld_out; }
        }
        q.layer_items[l] = ((grouped ? rows_max : p.total_rows) + 127) / 128 * j.nog;      // (128-row block) x (128-channel block) work items
    }
    q.kind = LAYERED;
    return SAD_OK;
}

// Geometry 1: narrow 3-layer grouped chains can run on the vector ALU (only on request: it computes the padding rows the tiled kernel
// skips; autotune tries it).  Launched from here.
static int prepare_valu(const Chain &c, sad_stream_t stream, Prepared &q) {
    const sad_mlp_args *a = c.a;
    const int *d = a->dims;
    int shape = 0;
    if (c.p.grouped && a->L == 3 && (a->relu_mask & 7) == 7 && d[0] == 4 && d[1] == 16 && d[2] == 16 && d[3] == 32) shape = 1;
    if (c.p.grouped && a->L == 3 && (a->relu_mask & 7) == 7 && d[0] == 4 && d[1] == 32 && d[2] == 32 && d[3] == 64) shape = 2;
    if (!shape) return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: no VALU kernel for this chain");
    ValuParams v{};
    v.xyz = a->xyz; v.new_xyz = a->new_xyz; v.feat = a->feat; v.idx = a->idx; v.cnt = a->cnt; v.out = a->out;
    for (int l = 0; l < 3; ++l) { v.w[l] = a->packed + c.g.raw_w[l]; v.b[l] = a->packed + c.g.raw_b[l]; }
    v.total_groups = c.p.total_groups; v.ld_feat = a->ld_feat; v.N = a->N; v.M = a->M; v.S = a->S;
    v.ld_out = a->ld_out; v.col_off = a->col_off; v.vec_out = c.p.vec_out;
    v.nodedup = sad::get_option(sad::OPT_MLP_NODEDUP);
    const long long gq = (long long)c.dedup_f * VALU_T / a->S;   // groups whose surviving rows fill ~one pass
    v.G = (int)(gq < 1 ? 1 : (gq > VALU_GMAX ? VALU_GMAX : gq));
    const long long nb = (c.p.total_groups + v.G - 1) / v.G;
    SAD_REQUIRE(nb < (1LL << 31), "sad_mlp_chain_f32: too many workgroups");
    q.kind = VALU_DONE;
    return launch_valu(v, shape, nb, (hipStream_t)stream);
}

// Every other geometry code: the tiled kernel, W waves of which WN = 1 << wn_shift lie along the output tiles, RW row tiles per wave
// (code 0: chosen here; else the digits W / wn_shift / RW).  Launches the row-packing scan itself when it packs rows globally.
static int prepare_tiled(const Chain &c, sad_stream_t stream, Prepared &q) {
    const sad_mlp_args *a = c.a;
    const Geometry &g = c.g;
    const bool grouped = c.p.grouped;
    const int dedup_f = c.dedup_f, flex_code = c.flex_code;
    MlpParams p = c.p;
    // LDS rows: bufA holds inputs of even layers / outputs of odd layers, bufB the others.  A layer's
    // output only needs the channels the next layer reads (its padded K).
    auto lds_rows = [&](int kc, int &ra, int &rb) {
        ra = kc; rb = 8;
        for (int l = 0; l + 1 < a->L; ++l) {  // the last layer's output never touches LDS
            int &dst = (l & 1) ? ra : rb;
            const int keep = g.kp[l + 1];
            dst = keep > dst ? keep : dst;
        }
    };
    int bias_total = 0;
    for (int l = 0; l < a->L; ++l) bias_total += g.np[l];
    p.bias_total = bias_total;
    // grouped mode: a workgroup owns G groups; with ball-query padding dropped their surviving rows
    // usually fit one pass of R rows (dedup_f = assumed ratio of padded to surviving rows)
    auto groups_per_wg = [&](int R) {
        long long gq = (long long)dedup_f * R / a->S;
        return (int)(gq < 1 ? 1 : (gq > 1024 ? 1024 : gq));
    };
    auto lds_bytes = [&](int w, int wns, int rw, int kcc) {
        int ra, rb;
        lds_rows(kcc, ra, rb);
        const size_t R = 32 * (size_t)rw * (w >> wns);
        const size_t G = grouped ? (size_t)groups_per_wg((int)R) : 0;
        const size_t nso = (G > R + 1 ? G : R + 1) + 2;     // s_off entries (static G+1, dynamic <= R+2) + broadcast slot
        return ((size_t)((ra + rb) / 4) * (4 * R + 8) + 2 * R + nso + (size_t)bias_total) * 4 + 16;
    };
    // ---- choose the workgroup geometry -----------------------------------------------------
    // W waves, WN along output tiles; R = 32*RW*(W/WN) rows per workgroup.
    const int bkb = sad::get_option(sad::OPT_MLP_BUDGET_KB);
    const size_t BUDGET2 = (size_t)(bkb > 0 ? bkb : 78) * 1024, BUDGET1 = 156 * 1024;
    int W = 8, wn_shift = 0, RW = 1, kc = g.kp[0];
    if (const int geom = c.geom_wg) {
        const int fw = geom / 100, fwns = (geom / 10) % 10, frw = geom % 10;
        const bool ok = (fw == 4 || fw == 8 || fw == 16) && (1 << fwns) <= fw && (frw == 1 || frw == 2 || frw == 4);
        if (!ok) return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry %d is not valid here", geom);
        W = fw; wn_shift = fwns; RW = frw;
        if (lds_bytes(W, wn_shift, RW, kc) > BUDGET1) {
            kc = g.kp[0] < 256 ? g.kp[0] : 256;
            if (kc == g.kp[0] || lds_bytes(W, wn_shift, RW, kc) > BUDGET1)
                return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: geometry %d does not fit LDS", geom);
        }
    } else {
        // Heuristic (PackedMLP.autotune measures instead): 8 waves; WN = flop-weighted mean number
        // of output tiles rounded down to a power of two (few idle waves, weights shared through
        // LDS rows rather than re-read per wave); then the most rows per wave that still leave two
        // workgroups per CU and at least two workgroups per CU-slot of work.
        double wsum = 0, fsum = 0;
        for (int l = 0; l < a->L; ++l) {
            const double f = (double)g.kp[l] * g.np[l];
            wsum += f * (g.np[l] / 32);
            fsum += f;
        }
        int wns0 = 0;
        while (wns0 < 3 && (2 << wns0) <= wsum / fsum + 1e-9) ++wns0;
        bool found = false;
        for (int pass = 0; pass < 3 && !found; ++pass) {
            const size_t budget = pass == 0 ? BUDGET2 : BUDGET1;
            const int kcc = pass < 2 ? g.kp[0] : (g.kp[0] < 256 ? g.kp[0] : 256);
            for (int wns = wns0; wns <= 3 && !found; ++wns) {
                int best_rw = 0;
                for (int rw = 4; rw >= 1; rw >>= 1) {
                    if (lds_bytes(8, wns, rw, kcc) > budget) continue;
                    if (!best_rw) best_rw = rw;   // largest that fits
                    const long long R = 32LL * rw * (8 >> wns);
                    const long long nb = grouped ? (p.total_groups * a->S / dedup_f + R - 1) / R : (p.total_rows + R - 1) / R;
                    if (nb >= 1024 || rw == 1) { best_rw = rw; break; }
                }
                if (best_rw) { wn_shift = wns; RW = best_rw; kc = kcc; found = true; }
            }
        }
        if (!found) return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: layer widths do not fit LDS");
    }
    p.wn_shift = wn_shift;
    if (flex_code > 3 || (flex_code && RW != 1))
        return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: flexible distribution / two tiles per wave need RW == 1");
    if ((flex_code & 2) && W == 16) return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: two tiles per wave: 4 or 8 waves");
    p.flex = flex_code & 1;
    p.kc = kc;
    lds_rows(kc, p.bufA_rows, p.bufB_rows);
    const size_t lds = lds_bytes(W, wn_shift, RW, kc);
    const long long R = 32LL * RW * (W >> wn_shift);
    p.G = grouped ? groups_per_wg((int)R) : 0;
    p.s_off_entries = (int)((p.G > R + 1 ? p.G : R + 1) + 1);
    p.nodedup = sad::get_option(sad::OPT_MLP_NODEDUP);
    p.rowtab = nullptr;
    long long grid_dyn = 0;
    long long macs_per_row = 0;
    for (int l = 0; l < a->L; ++l) macs_per_row += (long long)g.kp[l] * g.np[l];
    // global packing pays off when the prefix-sum workgroup is cheap (few groups) and rows are
    // expensive (measured: cluster.b1 +7 %, sa3.b2 +3 %, every small chain slower)
    const bool want_dyn = c.dyn_code == 1 || (c.dyn_code == 0 && p.total_groups <= 16384 && macs_per_row >= 400000);
    if (grouped && a->cnt && a->workspace && want_dyn && !sad::get_option(sad::OPT_MLP_STATIC)) {
        // global row packing: scan the counts once, then a persistent grid pulls full passes
        SAD_REQUIRE((uintptr_t)a->workspace % 16 == 0, "sad_mlp_chain_f32: workspace must be 16-byte aligned");
        SAD_REQUIRE(p.total_groups < (1LL << 30), "sad_mlp_chain_f32: too many groups");
        p.rowtab = (int *)a->workspace;
        if (int e = sad::launch_rowscan(a->cnt, (int)p.total_groups, a->S, (int)R, p.rowtab, (hipStream_t)stream, p.nodedup,
                                        a->idx, a->N, a->M)) return e;
        const sad::ScanLayout t = sad::scan_layout(p.total_groups, a->S);
        p.row_src = p.rowtab + t.row_src;
        p.row_gid = p.rowtab + t.row_gid;
        const long long upper = (p.total_groups * a->S + R - 1) / R;
        long long per_cu = lds > 80 * 1024 ? 1 : (lds > 52 * 1024 ? 2 : (lds > 39 * 1024 ? 3 : 4));
        if (sad::get_option(sad::OPT_MLP_DYN_SLOTS) > 0 && sad::get_option(sad::OPT_MLP_DYN_SLOTS) < per_cu)
            per_cu = sad::get_option(sad::OPT_MLP_DYN_SLOTS);
        grid_dyn = upper < 256 * per_cu ? upper : 256 * per_cu;
    }
    const long long nblocks = grid_dyn ? grid_dyn : (grouped ? (p.total_groups + p.G - 1) / p.G : (p.total_rows + R - 1) / R);
    SAD_REQUIRE(nblocks < (1LL << 31), "sad_mlp_chain_f32: too many workgroups");
    if (W == 16 && RW == 4) return sad::fail(SAD_EUNSUPPORTED, "sad_mlp_chain_f32: 16 waves support RW 1 or 2");
    q.kind = TILED;
    q.p = p; q.lds = lds; q.nblocks = nblocks; q.W = W; q.RW = RW; q.CW = (flex_code & 2) ? 2 : 1;
    if (!grid_dyn && !sad::get_option(sad::OPT_MLP_NOXCD)) {       // static chunks: XCD-aware order, grid padded to 8 * ceil(nb / 8)
        q.p.xcd_nb = (int)nblocks;
        q.nblocks = ((nblocks + 7) / 8) * 8;
    }
    return SAD_OK;
}

// Validation, then the preparer of the kernel the geometry code asks for; fills `q` for the launch.
static int prepare_chain(const sad_mlp_args *a, sad_stream_t stream, Prepared &q) {
    Chain c;
    if (int e = chain_args(a, c)) return e;
    q.prescanned = a->prescanned != 0;
    switch (c.geom_wg) {
    case 1: return prepare_valu(c, stream, q);
    case 2: case 4: return prepare_reg(c, q);
    case 3: return prepare_layered(c, q);
    case 5: return prepare_rows(c, q);
    default: return prepare_tiled(c, stream, q);
    }
}

namespace {
// scans of the chains that did not come with a table (prescanned = 0), in one pair of launches
int launch_pending_scans(const Prepared *const *qs, int n, hipStream_t st) {
    sad::ScanJob jobs[sad::REG_MAX_CHAINS];
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (!qs[i]->prescanned) jobs[m++] = qs[i]->scan;
    return m ? sad::launch_rowscan_multi(jobs, m, st) : SAD_OK;
}

int launch_reg_chains(const Prepared *const *qs, int n, hipStream_t st) {
    sad::RegMulti mp{};
    mp.n = n;
    mp.max_tiles = 0;
    if (int e = launch_pending_scans(qs, n, st)) return e;
    for (int i = 0; i < n; ++i) {
        mp.c[i] = qs[i]->rc;
        mp.shape[i] = qs[i]->reg_shape;
        mp.max_tiles += qs[i]->reg_tiles;
    }
    mp.counter = const_cast<int *>(mp.c[0].rowtab) + 2;      // zeroed by chain 0's rowscan
    mp.nq = qs[0]->scan.ngroups + 1 >= sad::ITEMQ_INTS ? 8 : 1;
    return qs[0]->kind == COOP ? sad::launch_coop(mp, st) : sad::launch_reg(mp, st);
}

// Layer-streamed chains (one or two with the same number of layers): one scan, then one
// launch per layer carrying that layer of every chain.
int launch_layered_chains(const Prepared *const *qs, int n, hipStream_t st) {
    if (int e = launch_pending_scans(qs, n, st)) return e;
    for (int l = 0; l < qs[0]->nl; ++l) {
        sad::LayerMulti lm{};
        lm.n = n;
        long long items = 0;
        for (int i = 0; i < n; ++i) { lm.j[i] = qs[i]->lj[l]; items += qs[i]->layer_items[l]; }
        // (items of a layer launch are dealt statically: pulling them from per-XCD queues as the cooperative kernel does
        // cost the pipeline 2.5 %)
        if (int e = sad::launch_layers(lm, items, st)) return e;
    }
    return SAD_OK;
}

int launch_prepared(const Prepared &q, hipStream_t st) {
    const Prepared *one = &q;
    switch (q.kind) {
    case VALU_DONE: return SAD_OK;
    case ROWS: return sad::launch_rows(q.rj, st);
    case LAYERED: return launch_layered_chains(&one, 1, st);
    case REG: case COOP: return launch_reg_chains(&one, 1, st);
    default: return launch_tiled(q.p, q.W, q.RW, q.CW, q.lds, q.nblocks, st);
    }
}
}  // namespace

SAD_API int sad_mlp_chain_f32(const sad_mlp_args *a, sad_stream_t stream) {
    Prepared q;
    if (int e = prepare_chain(a, stream, q)) return e;
    return launch_prepared(q, (hipStream_t)stream);
}

SAD_API int sad_mlp_chain_multi_f32(const sad_mlp_args *const *args, int n, sad_stream_t stream) {
    SAD_REQUIRE(args && n >= 1, "sad_mlp_chain_multi_f32: need at least one chain");
    hipStream_t st = (hipStream_t)stream;
    if (n > MULTI_MAX) {                       // more chains than one dispatch carries: in groups
        for (int i = 0; i < n; i += MULTI_MAX)
            if (int e = sad_mlp_chain_multi_f32(args + i, n - i < MULTI_MAX ? n - i : MULTI_MAX, stream)) return e;
        return SAD_OK;
    }
    Prepared q[MULTI_MAX];
    for (int i = 0; i < n; ++i)
        if (int e = prepare_chain(args[i], stream, q[i])) return e;
    // two layer-streamed chains with the same depth: their layers share launches (heavier chain first)
    if (n == 2 && q[0].kind == LAYERED && q[1].kind == LAYERED && q[0].nl == q[1].nl) {
        const int last = q[0].nl - 1;
        const bool swap = q[1].layer_items[last] * (long long)q[1].lj[last].kg > q[0].layer_items[last] * (long long)q[0].lj[last].kg;
        const Prepared *ord[2] = {swap ? &q[1] : &q[0], swap ? &q[0] : &q[1]};
        return launch_layered_chains(ord, 2, st);
    }
    double weight[MULTI_MAX];      // of a chain in a merged dispatch: MACs per row x rows (an upper bound)
    int order[MULTI_MAX];
    // register-resident chains (all cooperative or none) of one shape family: one dispatch, tiles of the heaviest chain first
    bool all_reg = n > 1 && n <= sad::REG_MAX_CHAINS && (q[0].kind == REG || q[0].kind == COOP);
    for (int i = 0; i < n; ++i) all_reg = all_reg && q[i].kind == q[0].kind && sad::reg_family(q[i].reg_shape) == sad::reg_family(q[0].reg_shape);
    if (all_reg) {
        for (int i = 0; i < n; ++i) {
            double m = 0;
            for (int l = 0; l < 3; ++l) m += (double)q[i].rc.np[l] * (l == 0 ? 8.0 * 17 : q[i].rc.np[l - 1]);
            weight[i] = m * (double)q[i].reg_tiles;
        }
        sad::heaviest_first(weight, n, order);
        const Prepared *ord[MULTI_MAX];
        for (int i = 0; i < n; ++i) ord[i] = &q[order[i]];
        return launch_reg_chains(ord, n, st);
    }
    // tiled chains with a common wave count (other than 16): one dispatch; otherwise one by one
    bool merge = n > 1;
    for (int i = 0; i < n; ++i) merge = merge && q[i].kind == TILED && q[i].W == q[0].W && q[i].W != 16;
    if (!merge) {
        for (int i = 0; i < n; ++i)
            if (int e = launch_prepared(q[i], st)) return e;
        return SAD_OK;
    }
    for (int i = 0; i < n; ++i) {
        double m = 0;
        for (int l = 0; l < q[i].p.L; ++l) m += (double)q[i].p.kp[l] * q[i].p.np[l];
        weight[i] = m * (double)q[i].p.total_rows;
    }
    sad::heaviest_first(weight, n, order);
    MultiParams mp{};
    mp.n = n;
    size_t lds = 0;
    long long total = 0;
    int rwmax = 1;
    for (int i = 0; i < n; ++i) {
        const Prepared &s = q[order[i]];
        mp.p[i] = s.p;
        mp.rw[i] = s.RW;
        mp.cw[i] = s.CW;
        mp.first[i] = (int)total;
        total += (s.nblocks + 7) / 8 * 8;          // chain starts stay multiples of 8 (XCD-aware chunk order)
        lds = s.lds > lds ? s.lds : lds;
        rwmax = s.RW > rwmax ? s.RW : rwmax;
    }
    SAD_REQUIRE(total < (1LL << 31), "sad_mlp_chain_multi_f32: too many workgroups");
    mp.first[n] = (int)total;
    bool cw2 = false;
    for (int i = 0; i < n; ++i) cw2 = cw2 || mp.cw[i] == 2;
    return launch_tiled_multi(mp, q[0].W, rwmax, cw2, lds, st);
}
