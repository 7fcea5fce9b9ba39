// rtg_rot_ingest.hip -- the zero-pose transforms of retarget/utils/parse_mocap.py:65-134 (zero_pose_transform.py:16-41
// is the same thing again) as ONE launch:
//   out[f, j] = qmul_norm(qmul_norm(q[f, src[j]], pre), post[j])
// pre is one axis rotation, post[j] = quat_inverse(t2zero[j]); src gathers the rows (the broadcast's 23 -> 21,
// sim_full_body_teleop.py:97-106, or the identity).  The reference normalises between the two products, so they are not
// folded into one, and pre's zero components are multiplied like any others (x * 0 decides -0, inf and NaN).
//
// One block of 16 T threads per tile of T frames: at most four records in and four items out per thread, whatever T.
// The tile's input rows are ONE contiguous span of T J_in 16-byte records: every thread issues all its loads of the span
// (record tid + 16 T k: 1 KiB per wave instruction, addresses clamped, not branched) and its piece of the handle's blob
// before the first LDS store; the records are staged in an LDS image of the tile.
// Item i = (frame i / J_out, joint i % J_out) reads row src[j] of its frame from the image and applies the two
// products with the FK family's device functions (qmul through the near-unit table, one rare-case branch per group of
// up to four items), so the bits are those of RTG_OP_QUAT_MUL_NORM applied twice.  AoS out (B, J_out, 4): item i IS output
// record i of the tile, whole-wave consecutive 16-byte stores.  SoA out (J_out, 4, B): the results go back into LDS
// (over the dead image) with an odd row stride 4 J_out + 1, and leave with the lanes on consecutive frames of a plane,
// like ingest_rows_out.  Plain stores: the solver launched next reads these rows.
//
// LDS: blob (1 + J_out + ceil(J_out / 4) + 33 units of 16 bytes: pre | post | src | the near-unit table) + the larger of
// the image (16 T J_in bytes) and, SoA, the result rows (4 T (4 J_out + 1) bytes).
#include "rtg_device.cuh"
#include "rtg_fk_group.cuh"

namespace rtg {

// the tile's items of the first N slots (item u NT + tid of slot u), as one N-way group: one rare-case branch each product
struct RotItems {
    const f4v *img, *post;
    const int *srcj;
    const UnitEnt *utab;
    Q pre;
    int Ji, Jo, nit;
    float rJ;
};
template <int N, int NT>
RTG_DEV void rot_items(const RotItems &P, int tid, Q (&r)[4])
{
    Q a[N], b[N], m[N], o[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        int i = u * NT + tid;
        i = i < P.nit ? i : 0;   // a lane past the tile repeats item 0
        const Item it = item_split(i, P.rJ, P.Jo);
        a[u] = q_of(P.img[it.fr * P.Ji + P.srcj[it.j]]);
        b[u] = P.pre;
        m[u] = q_of(P.post[it.j]);
    }
    qmul_norm_n<N>(a, b, o, fk_tab(P.utab));
    qmul_norm_n<N>(o, m, a, fk_tab(P.utab));
#pragma unroll
    for (int u = 0; u < N; ++u) r[u] = a[u];
}

// the near-unit table of a handle's blob: sqrt_clamp_rcp_exact's own values, as unit_tab_fill leaves them in LDS
__global__ __launch_bounds__(64) void k_rot_ingest_tab(UnitEnt *tab) { unit_tab_fill(tab, (int)threadIdx.x); }

template <int T, bool SOA>
__global__ __launch_bounds__(16 * T, 4) void k_rot_ingest(RotIngestView P, const float *__restrict__ q, int64_t B,
                                                    float *__restrict__ out)
{
    static_assert(T % 4 == 0 && T >= 8 && T <= 64, "whole waves; the blob in one pass; i / J through f32: i < 2^12");
    extern __shared__ __attribute__((aligned(16))) float ri_lds[];
    constexpr int NT = 16 * T;  // threads
    constexpr int NR = 4;       // records in, and items out, per thread: T * 64 / NT
    const int tid = (int)threadIdx.x;
    const int Ji = P.J_in, Jo = P.J_out;
    const int64_t f0 = (int64_t)blockIdx.x * T;
    const int nfr = (int)((B - f0) < T ? (B - f0) : T);
    f4v *cst = reinterpret_cast<f4v *>(ri_lds);
    f4v *img = cst + P.n16;

    // the tile's span and the blob, all loads in flight
    const f4v *span = reinterpret_cast<const f4v *>(q) + f0 * Ji;
    const int nrec = nfr * Ji;
    f4v v[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int rec = k * NT + tid;
        if (k * NT < nrec) v[k] = span[rec < nrec ? rec : 0];   // a uniform skip of the pieces past the tile
    }
    const f4v c = reinterpret_cast<const f4v *>(P.blob)[tid < P.n16 ? tid : 0];   // n16 <= 114
    if (tid < P.n16) cst[tid] = c;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int rec = k * NT + tid;
        if (rec < nrec) img[rec] = v[k];
    }
    __syncthreads();

    const int nit = nfr * Jo;
    const float rJ = item_rcp(Jo);
    const Q pre = q_of(cst[0]);
    const f4v *post = cst + 1;
    const int *srcj = reinterpret_cast<const int *>(cst + P.o_src);
    const UnitEnt *utab = reinterpret_cast<const UnitEnt *>(cst + P.o_tab);
    // a tile fills ceil(nit / NT) of the NR item slots (uniform: 23 -> 21 at T = 16 fills two): only those are computed
    Q r[NR];
    const RotItems it{img, post, srcj, utab, pre, Ji, Jo, nit, rJ};
    switch ((nit + NT - 1) / NT) {
    case 1: rot_items<1, NT>(it, tid, r); break;
    case 2: rot_items<2, NT>(it, tid, r); break;
    case 3: rot_items<3, NT>(it, tid, r); break;
    default: rot_items<4, NT>(it, tid, r); break;
    }

    if (!SOA) {
        f4v *dst = reinterpret_cast<f4v *>(out) + f0 * Jo;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int i = k * NT + tid;
            if (i < nit) dst[i] = v_of(r[k]);
        }
    } else {
        const int RS = 4 * Jo + 1;
        float *res = reinterpret_cast<float *>(img);
        __syncthreads();   // every item has read the image: the result rows take its place
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int i = k * NT + tid;
            if (i < nit) {
                const Item it = item_split(i, rJ, Jo);
                float *d = res + it.fr * RS + 4 * it.j;
                d[0] = r[k].x, d[1] = r[k].y, d[2] = r[k].z, d[3] = r[k].w;
            }
        }
        __syncthreads();
        const int n = 4 * Jo * T;
        for (int e = tid; e < n; e += NT) {
            const int plane = e / T, fr = e - plane * T;
            if (fr < nfr) out[(int64_t)plane * B + f0 + fr] = res[fr * RS + plane];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host
void rot_ingest_blob(int32_t J_in, int32_t J_out, const int32_t *src, const float *pre, const float *post,
                     std::vector<float> &blob, RotIngestView &V_)
{
    V_.J_in = J_in, V_.J_out = J_out;
    V_.o_src = 1 + J_out;
    V_.o_tab = V_.o_src + (J_out + 3) / 4;
    V_.n16 = V_.o_tab + (2 * kUnitTabK + 1);
    static_assert(sizeof(UnitEnt) == 16, "the near-unit table in 16-byte units");
    blob.assign((size_t)4 * V_.n16, 0.0f);
    memcpy(blob.data(), pre, sizeof(float) * 4);
    memcpy(blob.data() + 4, post, sizeof(float) * 4 * J_out);
    int32_t *ip = reinterpret_cast<int32_t *>(blob.data() + 4 * V_.o_src);
    for (int j = 0; j < J_out; ++j) ip[j] = src ? src[j] : j;
}

hipError_t launch_rot_ingest_tab(float *blob_tab, hipStream_t s)
{
    hipLaunchKernelGGL(k_rot_ingest_tab, dim3(1), dim3(64), 0, s, reinterpret_cast<UnitEnt *>(blob_tab));
    return hipGetLastError();
}

template <int T, bool SOA>
static size_t rot_ingest_lds(const RotIngestView &P)
{
    const size_t image = (size_t)16 * T * P.J_in, rows = SOA ? (size_t)4 * T * (4 * P.J_out + 1) : 0;
    return (size_t)16 * P.n16 + (((image > rows ? image : rows) + 15) & ~(size_t)15);
}

hipError_t launch_rot_ingest(const RotIngestView &P, const float *q, int64_t B, int layout, float *out, hipStream_t s)
{
    // the largest request (J_in = J_out = 64) stays under the 64 KB a launch may ask for without an attribute
    static_assert(16 * 114 + 16 * kRotIngAosTile * kRotIngMaxJ <= 65536, "AoS tile too large for LDS");
    static_assert(16 * 114 + 4 * kRotIngSoaTile * (4 * kRotIngMaxJ + 1) <= 65536, "SoA tile too large for LDS");
    if (layout == RTG_LAYOUT_SOA) {
        const size_t lds = rot_ingest_lds<kRotIngSoaTile, true>(P);
        hipLaunchKernelGGL((k_rot_ingest<kRotIngSoaTile, true>), dim3(grid_for(B, kRotIngSoaTile)), dim3(16 * kRotIngSoaTile), lds, s,
                           P, q, B, out);
    } else {
        const size_t lds = rot_ingest_lds<kRotIngAosTile, false>(P);
        hipLaunchKernelGGL((k_rot_ingest<kRotIngAosTile, false>), dim3(grid_for(B, kRotIngAosTile)), dim3(16 * kRotIngAosTile), lds, s,
                           P, q, B, out);
    }
    return hipGetLastError();
}

}  // namespace rtg
