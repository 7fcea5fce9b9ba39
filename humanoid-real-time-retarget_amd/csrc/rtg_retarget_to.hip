// rtg_retarget_to.hip -- SkeletonState.retarget_to (poselib skeleton3d.py:742-889) as ONE launch on the lane groups of
// rtg_fk_group.cuh, and the host tables / schedules of its plan.
//
// With S the source tree (Js joints), T the target tree (Jt), K mapped (source, target) pairs, S_red / T_red the trees
// with only the mapped joints kept (drop_nodes_by_names, :226-259), R = rotation_to_target_skeleton and s the scale,
// a frame goes through (every from_rotation_and_root_translation of the reference normalises; those stay):
//   1. Gs = the source state's global rotations: state FK over S with S's tree quaternions (:402-425) for a local
//      state, on a list schedule pruned to the mapped joints' ancestors; the rows as stored for a global state;
//   2. g = normalize(Gs[kept])                                                       (_transfer_to, :676-683)
//   3. l_k = qmul_norm(normalize(conj(identity)), qmul_norm(conj(g_parent), g_k)) over S_red, root copied (:460-484)
//   4. permute to T_red's order, normalize                                           (_remapped_to, :721-740)
//   5. l_0 = qmul_norm(R, l_0), normalize; t' = quat_rotate(R, root_t)               (:848-855)
//   6. state FK of l over T_red with identity tree quaternions -> G                  (:868, through :402-425)
//   7. n = qmul_norm(qmul_norm(G, conj(G_tp)), TG)                                   (:868-869)
//   8. o_j = normalize(n[src_of[j]]) for T's Jt joints                               (:876-886)
//   9. inverse FK over T with T's tree quaternions, normalize: the output rows       (.local_repr(), :636-650)
//  10. root = tgt_tpose_root + (t' - t'_tp) f32(s)                                   (:858, :885)
// G_tp (stages 1-6 of the source t-pose) and TG (the target t-pose's global rotations at the mapped joints) are the
// plan's constants, evaluated on the device at plan creation (rtg_api.cpp) by this kernel and the FK kernel.
//
// A tile is one wave and F frames (group_frames(max(Js, Jt))), 64 / F lanes per frame.  The source rows come in as
// coalesced 1 KiB pieces into an LDS image, all loads in flight; stages 1 and 6 run the schedules' steps on the
// frame's lane group, the other stages have no chain and spread their (frame, joint) items over the wave; the output
// rows leave as whole-wave non-temporal stores.  LDS: RetargetImages below (the stage-3..6 rows overlay the image, dead
// after stage 2; stage 8's rows are stage 7's, indexed through src_of; the blob holds the schedules, constants and
// index tables).  Each joint is composed by the device functions the
// FK kernels use (qmul_norm through the near-unit table, qnormalize, qrotate) with the reference's operands in the
// reference's order, so the bits do not depend on the schedule or on which lane does what.
#include "rtg_device.cuh"
#include "rtg_fk_group.cuh"
#include "rtg_group_sched.h"

namespace rtg {

// a list schedule's steps on the rotations alone: joint j's row becomes qmul_norm(parent's global row,
// qmul_norm(tree quaternion, row)) (:416-422); the root's row is its global rotation already and has no entry
template <int F>
RTG_DEV void rot_compose(f4v *img, int stride, const GEnt *sch, int steps, int nfr, const UnitEnt *utab)
{
    using G = Grp<F>;
    const int lane = (int)threadIdx.x;
    const int fr = lane >> G::LOG_L, sub = lane & (G::L - 1);
    const bool live = fr < nfr;
    const int base = fr * stride;
    for (int s = 0; s < steps; ++s) {
        const GEnt e = sch[s * G::L + sub];
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (live && j != 0xFF) {
            const Q lq = qmul_norm(Q{e.qx, e.qy, e.qz, e.qw}, q_of(img[base + j]), fk_tab(utab));
            img[base + j] = v_of(qmul_norm(q_of(img[base + p]), lq, fk_tab(utab)));
        }
        wave_sync();   // this step's rows before the next step's parent reads (other lanes)
    }
}

struct RetargetImages {
    f4v *img;        // [F Js] the source rows; dead after stage 2, its rows [F K] then take stages 3-6
    f4v *red;        // [F K] the reduced rows
    f4v *tab;        // [n16] the plan's blob
    UnitEnt *utab;   // the near-unit table
    size_t floats;
    __host__ __device__ RetargetImages(float *base, const RetargetView &P)
    {
        LdsCarve c(base);
        img = c.take<f4v>((size_t)P.F * P.Js);
        red = c.take<f4v>((size_t)P.F * P.K);
        tab = c.take<f4v>(P.n16);
        utab = c.take_unit_tab();
        floats = c.floats;
    }
};

template <bool LOCAL_IN, int F>
__global__ __launch_bounds__(64, 4) void k_retarget_to(RetargetView P, const float *__restrict__ src_rot,
                                                       const float *__restrict__ src_root_t, int64_t B,
                                                       float *__restrict__ out_rot, float *__restrict__ out_root_t,
                                                       float *__restrict__ dump)
{
    extern __shared__ __attribute__((aligned(16))) float rt_lds[];
    using G = Grp<F>;
    const int lane = (int)threadIdx.x;
    const int Js = P.Js, Jt = P.Jt, K = P.K;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(B, f0);
    const RetargetImages I(rt_lds, P);
    f4v *img = I.img, *red = I.red, *tab = I.tab;
    const GEnt *sch1 = reinterpret_cast<const GEnt *>(tab);
    const GEnt *sch6 = reinterpret_cast<const GEnt *>(tab + P.o_sch6);
    const f4v *cg = tab + P.o_cg, *tg = tab + P.o_tg, *ttqn = tab + P.o_ttq;
    const int *kept = reinterpret_cast<const int *>(tab + P.o_int);
    const int *spar = kept + K, *perm = spar + K, *src_of = perm + K, *tpar = src_of + Jt;
    UnitEnt *utab = I.utab;

    // the tile's rows and root translations, all loads in flight; the plan's blob and the near-unit table meanwhile
    GroupRows<F> rows;
    rows.load(src_rot + f0 * Js * 4, nfr * Js);
    const float *rp = src_root_t + (f0 + (lane < nfr ? lane : 0)) * 3;
    const V root{rp[0], rp[1], rp[2]};
    {
        const f4v *gb = reinterpret_cast<const f4v *>(P.blob);
        for (int i = lane; i < P.n16; i += 64) {
            f4v v = gb[i];
            if (i >= P.o_ttq && i < P.o_ttq + Jt) v = v_of(qnormalize(qconj(q_of(v))));   // :477-478, once per joint
            tab[i] = v;
        }
    }
    if (kUnitTab) unit_tab_fill(utab, lane);
    rows.store(img, nfr * Js);
    wave_sync();

    if (LOCAL_IN) rot_compose<F>(img, Js, sch1, P.steps1, nfr, utab);   // stage 1

    const int nk = nfr * K;
    const float rK = item_rcp(K);
    for (int i = lane; i < nk; i += 64) {   // stage 2
        const Item it = item_split(i, rK, K);
        red[i] = v_of(qnormalize(q_of(img[it.fr * Js + kept[it.j]]), fk_tab(utab)));
    }
    wave_sync();   // the image is dead from here: rows [F K] of it take stages 3-6
    const Q cid = qnormalize(qconj(qident()));   // S_red's tree quaternions are identities (:259, :477-481)
    for (int i = lane; i < nk; i += 64) {   // stages 3-5
        const Item it = item_split(i, rK, K);
        const int fr = it.fr, k = it.j, ks = perm[k];
        const Q g = q_of(red[fr * K + ks]);
        Q l = g;   // S_red's root copied (:470)
        if (ks > 0) {
            l = qmul_norm(qconj(q_of(red[fr * K + spar[ks]])), g, fk_tab(utab));
            l = qmul_norm(cid, l, fk_tab(utab));
        }
        l = qnormalize(l, fk_tab(utab));                      // :735-740
        if (k == 0) l = qmul_norm(P.R, l, fk_tab(utab));      // :849
        img[i] = v_of(qnormalize(l, fk_tab(utab)));           // :850-855
    }
    const V tr = qrotate(P.R, root);                     // :853
    wave_sync();

    rot_compose<F>(img, K, sch6, P.steps6, nfr, utab);   // stage 6

    if (dump) {   // plan creation's t-pose pass (B = 1): G and t' of frame 0, nothing else
        f4v *dg = reinterpret_cast<f4v *>(dump);
        for (int i = lane; i < K; i += 64) dg[i] = img[i];
        if (lane == 0) {
            dump[4 * K] = tr.x;
            dump[4 * K + 1] = tr.y;
            dump[4 * K + 2] = tr.z;
        }
        return;
    }

    for (int i = lane; i < nk; i += 64) {   // stage 7, and stage 8's normalisation (the same for every j it serves)
        const int k = item_split(i, rK, K).j;
        const Q d = qmul_norm(q_of(img[i]), q_of(cg[k]), fk_tab(utab));
        const Q n = qmul_norm(d, q_of(tg[k]), fk_tab(utab));
        red[i] = v_of(qnormalize(n, fk_tab(utab)));
    }
    wave_sync();

    if (lane < nfr) {   // stage 10
        float *o = out_root_t + (f0 + lane) * 3;
        o[0] = P.tgt_root.x + (tr.x - P.t_tp.x) * P.scale;
        o[1] = P.tgt_root.y + (tr.y - P.t_tp.y) * P.scale;
        o[2] = P.tgt_root.z + (tr.z - P.t_tp.z) * P.scale;
    }
    const int nrec = nfr * Jt;
    const float rJ = item_rcp(Jt);
    f4v *dst = reinterpret_cast<f4v *>(out_rot + f0 * Jt * 4);
#pragma unroll 3
    for (int k = 0; k < G::NR; ++k) {   // stages 8-9, record-ordered: whole-wave stores
        const int rec = k * 64 + lane;
        if (rec < nrec) {
            const Item it = item_split(rec, rJ, Jt);
            const int fr = it.fr, j = it.j;
            const Q o = q_of(red[fr * K + src_of[j]]);
            Q q = o;   // T's root copied (:470)
            if (j > 0) {
                q = qmul_norm(qconj(q_of(red[fr * K + src_of[tpar[j]]])), o, fk_tab(utab));
                q = qmul_norm(q_of(ttqn[j]), q, fk_tab(utab));
            }
            st_out(dst + rec, v_of(qnormalize(q, fk_tab(utab))));   // :645-650
        }
    }
}

// ---------------------------------------------------------------------------------------------------- fit targets
// Keypoint targets for the pose fit (rtg.h rtg_fit_targets_*): Retarget.rescale_motion_to_standard_size (main.py:37-47)
// across two trees joined by K (source joint, target link) pairs.  A tile is one wave and F frames.  The source rows
// come in as coalesced pieces into an LDS image; every (frame, pair) item then writes its own term into the output
// image's row t_k -- the root pair its row, any other pair d / scale, k_rescale_motion's expressions on the pair's
// source rows and its target segment -- and the rows are summed level by level of the reduced target tree,
// out[t_k] = out[t_a(k)] + term, so every row is the one chain of additions taken parents first whichever lane does
// it; the unmapped links copy their nearest mapped ancestor's row and the image leaves as whole-wave non-temporal
// stores.  LDS: FitTargetsImages, 12 F (Js + Jt) + 16 K + 4 Jt bytes.
struct FitTargetsImages {
    float *src;   // [F Js 3] the source rows
    float *out;   // [F Jt 3] the target rows
    f4v *tab;     // [K] {norm(seg), -, -, code}
    int *cp;      // [Jt] the row link j copies (its own when mapped)
    size_t floats;
    __host__ __device__ FitTargetsImages(float *base, const FitTargetsView &P)
    {
        LdsCarve c(base);
        src = c.take<float>((size_t)3 * P.F * P.Js);
        out = c.take<float>((size_t)3 * P.F * P.Jt);
        tab = c.take<f4v>(P.K);
        cp = c.take<int>(P.Jt);
        floats = c.floats;
    }
};

template <int F>
__global__ __launch_bounds__(64) void k_fit_targets(FitTargetsView P, const float *__restrict__ src_pos, int64_t B,
                                                    float *__restrict__ target_pos)
{
    extern __shared__ __attribute__((aligned(16))) float ft_lds[];
    const int lane = (int)threadIdx.x;
    const int Js = P.Js, Jt = P.Jt, K = P.K;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(B, f0);
    const FitTargetsImages I(ft_lds, P);
    float *src = I.src, *out = I.out;
    f4v *tab = I.tab;
    int *cp = I.cp;

    // the tile's rows, all loads in flight; the plan's tables meanwhile (a segment's norm once per tile)
    const float *g_src = src_pos + f0 * Js * 3;
    PosRows<F> rows;
    rows.load(g_src, 3 * nfr * Js);
    {
        const f4v *gb = reinterpret_cast<const f4v *>(P.blob);
        for (int i = lane; i < K; i += 64) {
            f4v e = gb[i];
            e.x = lnorm3(V{e.x, e.y, e.z});
            tab[i] = e;
        }
        const int *gc = reinterpret_cast<const int *>(gb + K);
        for (int j = lane; j < Jt; j += 64) cp[j] = gc[j];
    }
    rows.to_lds(src, g_src, 3 * nfr * Js);
    wave_sync();

    auto mp = [&](const float *p) {   // coord_transform(dir) (main.py:170)
        const V v{p[0], p[1], p[2]};
        return P.dir_on ? V{v.x * P.dir.x, v.y * P.dir.y, v.z * P.dir.z} : v;
    };
    const int nk = nfr * K;
    const float rK = item_rcp(K);
    for (int i = lane; i < nk; i += 64) {   // every pair's own term
        const Item it = item_split(i, rK, K);
        const f4v e = tab[it.j];
        const int code = __float_as_int(e.w);
        const int sk = code & 63, sa = (code >> 6) & 63, tk = (code >> 12) & 63, depth = (code >> 24) & 63;
        const float *sf = src + 3 * it.fr * Js;
        V r = mp(sf + 3 * sk);
        if (depth == 0) {   // the root pair
            if (P.scale_on) r = V{r.x * P.root_scale.x, r.y * P.root_scale.y, r.z * P.root_scale.z};
            if (P.offset_on) r = V{r.x + P.root_offset.x, r.y + P.root_offset.y, r.z + P.root_offset.z};
        } else {
            const V d = vsub(r, mp(sf + 3 * sa));
            const float scale = lnorm3(d) / e.x;
            r = vdiv(d, scale);
        }
        float *o = out + 3 * (it.fr * Jt + tk);
        o[0] = r.x; o[1] = r.y; o[2] = r.z;
    }
    wave_sync();
    for (int lv = 1; lv <= P.levels; ++lv) {   // parents first: a level's anchors are all of lower levels
        for (int i = lane; i < nk; i += 64) {
            const Item it = item_split(i, rK, K);
            const int code = __float_as_int(tab[it.j].w);
            if (((code >> 24) & 63) != lv) continue;
            float *o = out + 3 * (it.fr * Jt + ((code >> 12) & 63));
            const float *a = out + 3 * (it.fr * Jt + ((code >> 18) & 63));
            o[0] = a[0] + o[0]; o[1] = a[1] + o[1]; o[2] = a[2] + o[2];
        }
        wave_sync();
    }
    const int nj = nfr * Jt;
    const float rJ = item_rcp(Jt);
    for (int i = lane; i < nj; i += 64) {   // the unmapped links
        const Item it = item_split(i, rJ, Jt);
        const int c = cp[it.j];
        if (c == it.j) continue;
        float *o = out + 3 * i;
        const float *a = out + 3 * (it.fr * Jt + c);
        o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
    }
    wave_sync();
    PosRows<F>::out(out, target_pos + f0 * Jt * 3, 3 * nj);
}

// ---------------------------------------------------------------------------------------------------- host
static void reduce_tree(const int32_t *parents, int32_t J, const std::vector<char> &keep, std::vector<int32_t> &kept,
                        std::vector<int32_t> &red_par)
{
    std::vector<int32_t> new_index(J, -1);
    for (int j = 0; j < J; ++j) {
        if (!keep[j]) continue;
        int p = parents[j];
        while (p != -1 && !keep[p]) p = parents[p];
        new_index[j] = (int32_t)kept.size();
        kept.push_back(j);
        red_par.push_back(p == -1 ? -1 : new_index[p]);
    }
}

bool retarget_tables(const int32_t *sp, int32_t Js, const int32_t *tp, int32_t Jt, const int32_t *sj,
                     const int32_t *tj, int32_t K, RetargetTables &out, std::string &err)
{
    char buf[160];
    if (Js < 1 || Jt < 1 || Js > kGroupMaxJ || Jt > kGroupMaxJ) {
        snprintf(buf, sizeof buf, "retarget_to serves trees of 1..%d joints (source %d, target %d)", kGroupMaxJ, Js, Jt);
        err = buf;
        return false;
    }
    if (K < 1 || !sj || !tj) {
        err = "the joint mapping is empty";
        return false;
    }
    std::vector<char> ks(Js, 0), kt(Jt, 0);
    std::vector<int32_t> src_for(Jt, -1);
    for (int i = 0; i < K; ++i) {
        if (sj[i] < 0 || sj[i] >= Js || tj[i] < 0 || tj[i] >= Jt) {
            snprintf(buf, sizeof buf, "mapping pair %d = (%d, %d) is out of range (source %d, target %d joints)", i,
                     sj[i], tj[i], Js, Jt);
            err = buf;
            return false;
        }
        if (ks[sj[i]] || kt[tj[i]]) {   // :729: the reduced trees would not have K joints each
            err = "the joint mapping is not consistent with the skeleton trees";
            return false;
        }
        ks[sj[i]] = kt[tj[i]] = 1;
        src_for[tj[i]] = sj[i];
    }
    if (!ks[0] || !kt[0]) {
        err = "the root node cannot be dropped";   // :243
        return false;
    }
    out = RetargetTables{};
    out.Js = Js, out.Jt = Jt, out.K = K;
    reduce_tree(sp, Js, ks, out.kept_s, out.sred_par);
    reduce_tree(tp, Jt, kt, out.kept_t, out.tred_par);
    std::vector<int32_t> s_index(Js, -1), t_index(Jt, -1);
    for (int k = 0; k < K; ++k) s_index[out.kept_s[k]] = k, t_index[out.kept_t[k]] = k;
    out.perm.resize(K);
    for (int k = 0; k < K; ++k) out.perm[k] = s_index[src_for[out.kept_t[k]]];
    out.src_of.resize(Jt);
    for (int j = 0; j < Jt; ++j) {
        int a = j;
        while (!kt[a]) a = tp[a];   // ends at the root, which is mapped
        out.src_of[j] = t_index[a];
    }
    return true;
}

// a list schedule's entries for rot_compose: joint, parent and the joint's tree quaternion (no child links)
static int rot_schedule(const int32_t *par, int J, const char *inc, int L, const Q *tq, std::vector<GEnt> &out)
{
    std::vector<int> order;
    const int steps = group_list_schedule(par, J, inc, false, L, J, order);
    for (const int j : order)
        out.push_back(j < 0 ? GEnt{0.f, 0.f, 0.f, 0xFFFF, 0.f, 0.f, 0.f, 1.f}
                            : GEnt{0.f, 0.f, 0.f, (int32_t)((uint32_t)j | ((uint32_t)par[j] << 8)), tq[j].x, tq[j].y,
                                   tq[j].z, tq[j].w});
    return steps;
}

void retarget_blob(const RetargetTables &T, const int32_t *sp, const Q *stq, const int32_t *tp, const Q *ttq,
                   std::vector<float> &blob, RetargetView &V_)
{
    const int Js = T.Js, Jt = T.Jt, K = T.K;
    const int F = group_frames(std::max(Js, Jt)), L = 64 / F;
    std::vector<char> inc(Js, 0);   // stage 1: the mapped joints' ancestors
    for (int k = 0; k < K; ++k)
        for (int a = T.kept_s[k]; a != -1 && !inc[a]; a = sp[a]) inc[a] = 1;
    std::vector<GEnt> s1, s6;
    const int steps1 = rot_schedule(sp, Js, inc.data(), L, stq, s1);
    const std::vector<Q> ident(K, Q{0.f, 0.f, 0.f, 1.f});
    const int steps6 = rot_schedule(T.tred_par.data(), K, nullptr, L, ident.data(), s6);
    V_.Js = Js, V_.Jt = Jt, V_.K = K, V_.F = F, V_.steps1 = steps1, V_.steps6 = steps6;
    V_.o_sch6 = 2 * (int)s1.size();
    V_.o_cg = V_.o_sch6 + 2 * (int)s6.size();
    V_.o_tg = V_.o_cg + K;
    V_.o_ttq = V_.o_tg + K;
    V_.o_int = V_.o_ttq + Jt;
    const int nint = 3 * K + 2 * Jt;
    V_.n16 = V_.o_int + (nint + 3) / 4;
    blob.assign((size_t)4 * V_.n16, 0.0f);
    if (!s1.empty()) memcpy(blob.data(), s1.data(), sizeof(GEnt) * s1.size());
    if (!s6.empty()) memcpy(blob.data() + 4 * V_.o_sch6, s6.data(), sizeof(GEnt) * s6.size());
    memcpy(blob.data() + 4 * V_.o_ttq, ttq, sizeof(Q) * Jt);
    int32_t *ip = reinterpret_cast<int32_t *>(blob.data() + 4 * V_.o_int);
    for (int k = 0; k < K; ++k) ip[k] = T.kept_s[k], ip[K + k] = T.sred_par[k] < 0 ? 0 : T.sred_par[k], ip[2 * K + k] = T.perm[k];
    for (int j = 0; j < Jt; ++j) ip[3 * K + j] = T.src_of[j], ip[3 * K + Jt + j] = tp[j] < 0 ? 0 : tp[j];
}

hipError_t launch_retarget_to(const RetargetView &P, bool local_in, const float *rot, const float *root_t, int64_t B,
                              float *out_rot, float *out_root_t, float *dump, hipStream_t s)
{
    const size_t lds = sizeof(float) * RetargetImages(nullptr, P).floats;
    group_dispatch(P.F, [&](auto f, auto li) {
        hipLaunchKernelGGL((k_retarget_to<li(), f()>), dim3(grid_for(B, P.F)), dim3(64), lds, s, P, rot, root_t, B, out_rot,
                           out_root_t, dump);
    }, local_in);
    return hipGetLastError();
}

bool fit_targets_tables(int32_t Js, const int32_t *tp, const float *tlt, int32_t Jt, const int32_t *sj,
                        const int32_t *tj, int32_t K, FitTargetsTables &out, std::string &err)
{
    char buf[160];
    if (Js < 1 || Jt < 1 || Js > kGroupMaxJ || Jt > kGroupMaxJ) {
        snprintf(buf, sizeof buf, "fit targets serve trees of 1..%d joints (source %d, target %d)", kGroupMaxJ, Js, Jt);
        err = buf;
        return false;
    }
    if (K < 1 || !sj || !tj) {
        err = "the joint mapping is empty";
        return false;
    }
    std::vector<int32_t> pair_of(Jt, -1), seen_s(Js, -1);
    for (int i = 0; i < K; ++i) {
        if (sj[i] < 0 || sj[i] >= Js || tj[i] < 0 || tj[i] >= Jt) {
            snprintf(buf, sizeof buf, "mapping pair %d = (%d, %d) is out of range (source %d, target %d joints)", i,
                     sj[i], tj[i], Js, Jt);
            err = buf;
            return false;
        }
        if (seen_s[sj[i]] >= 0 || pair_of[tj[i]] >= 0) {
            const bool s = seen_s[sj[i]] >= 0;
            snprintf(buf, sizeof buf, "%s joint %d is named twice (pairs %d and %d)", s ? "source" : "target",
                     s ? sj[i] : tj[i], s ? seen_s[sj[i]] : pair_of[tj[i]], i);
            err = buf;
            return false;
        }
        seen_s[sj[i]] = pair_of[tj[i]] = i;
    }
    if (pair_of[0] < 0) {
        err = "the target root is not mapped";
        return false;
    }
    out = FitTargetsTables{};
    out.Js = Js, out.Jt = Jt, out.K = K;
    std::vector<float> G((size_t)3 * Jt, 0.0f);   // the zero pose's global translations, parents first, G[root] = 0
    for (int j = 1; j < Jt; ++j)
        for (int c = 0; c < 3; ++c) G[3 * j + c] = G[3 * tp[j] + c] + tlt[3 * j + c];
    out.src_of.resize(Jt);
    out.weight.resize(Jt);
    for (int j = 0; j < Jt; ++j) {
        int a = j;
        while (pair_of[a] < 0) a = tp[a];   // ends at the root, which is mapped
        out.src_of[j] = pair_of[a];
        out.weight[j] = pair_of[j] >= 0 ? 1.0f : 0.0f;
    }
    out.anchor.assign(K, -1);
    out.depth.assign(K, 0);
    out.seg.assign((size_t)3 * K, 0.0f);
    for (int j = 1; j < Jt; ++j) {   // ascending target index: an anchor's depth is there before its pairs ask
        const int k = pair_of[j];
        if (k < 0) continue;
        const int a = out.src_of[tp[j]], ta = tj[a];
        out.anchor[k] = a;
        out.depth[k] = out.depth[a] + 1;
        out.levels = std::max(out.levels, out.depth[k]);
        for (int c = 0; c < 3; ++c) out.seg[3 * k + c] = G[3 * j + c] - G[3 * ta + c];
    }
    return true;
}

void fit_targets_blob(const FitTargetsTables &T, const int32_t *sj, const int32_t *tj, std::vector<float> &blob,
                      FitTargetsView &V_)
{
    const int K = T.K, Jt = T.Jt;
    V_.Js = T.Js, V_.Jt = Jt, V_.K = K, V_.F = group_frames(std::max(T.Js, Jt)), V_.levels = T.levels;
    blob.assign((size_t)4 * K + (size_t)((Jt + 3) & ~3), 0.0f);
    for (int k = 0; k < K; ++k) {
        const int a = T.anchor[k] < 0 ? k : T.anchor[k];
        const int32_t code = sj[k] | (sj[a] << 6) | (tj[k] << 12) | (tj[a] << 18) | (T.depth[k] << 24);
        memcpy(&blob[4 * (size_t)k], &T.seg[3 * (size_t)k], sizeof(float) * 3);
        memcpy(&blob[4 * (size_t)k + 3], &code, sizeof code);
    }
    int32_t *cp = reinterpret_cast<int32_t *>(blob.data() + 4 * (size_t)K);
    for (int j = 0; j < Jt; ++j) cp[j] = tj[T.src_of[j]];
}

hipError_t launch_fit_targets(const FitTargetsView &P, const float *src_pos, int64_t B, float *target_pos, hipStream_t s)
{
    const size_t lds = sizeof(float) * FitTargetsImages(nullptr, P).floats;
    group_dispatch(P.F, [&](auto f) {
        hipLaunchKernelGGL((k_fit_targets<f()>), dim3(grid_for(B, P.F)), dim3(64), lds, s, P, src_pos, B, target_pos);
    });
    return hipGetLastError();
}

}  // namespace rtg
