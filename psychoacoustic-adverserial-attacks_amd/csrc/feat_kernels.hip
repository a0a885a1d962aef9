// The label-free feature-distance loss: cosine distance between the rows of two hidden states, with its cotangent.
//
//   d[b][t]  = 1 - <h, r> / (|h| |r|)                          loss_b = sum_{t < T_b} d[b][t]
//   dh[b][t] = -grad_scale (r / |r| - cos h / |h|) / |h|       zero rows for t >= T_b and for the pad rows t >= T
//
// A row with |h| <= 1e-8 or |r| <= 1e-8 has d = 1 and a zero cotangent row: this is the definition (tests/feature_ref.py states the
// same).  The three dot products are accumulated in double from the f32 inputs, d is rounded to f32 once, and loss_b is the double
// sum of those f32 values in a fixed order, rounded once.  No atomics: two calls give the same bits.
#include "model_kernels.h"

namespace paa {

namespace {

constexpr double FEAT_EPS = 1e-8;

// the clip's frame count, clamped to [1, T] so a bad entry never indexes out of bounds (null: T)
__device__ __forceinline__ int feat_frames(const int32_t* __restrict__ frames, int b, int T) {
    if (!frames) return T;
    const int v = frames[b];
    return v < 1 ? 1 : (v > T ? T : v);
}

// One wave per row of the (B, h_rows) row space of h / dh; rows t >= T only receive their zero cotangent row.  VEC: 16-byte
// loads and stores (every pointer 16-byte aligned; H % 4 == 0 keeps the rows so); else dword accesses.  The first 1024 columns of
// both rows stay in registers between the two passes, as in k_ln_fwd; wider rows re-read the rest (L1 / L2 hits).
template <bool VEC>
__global__ __launch_bounds__(256) void k_feat_cos(const float* __restrict__ h, int h_rows, const float* __restrict__ ref, int ref_rows,
                                                  const int32_t* __restrict__ frames, int B, int T, int H, float grad_scale,
                                                  float* __restrict__ dwork, float* __restrict__ dist, float* __restrict__ dh,
                                                  int rows_per_clip) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (int64_t)B * rows_per_clip) return;
    const int b = (int)(row / rows_per_clip), t = (int)(row - (int64_t)b * rows_per_clip);
    float* dr = dh ? dh + ((size_t)b * h_rows + t) * H : nullptr;
    auto load4 = [&](const float* p) -> float4 {
        if (VEC) return *reinterpret_cast<const float4*>(p);
        return make_float4(p[0], p[1], p[2], p[3]);
    };
    auto store4 = [&](float* p, const float4& v) {
        if (VEC) *reinterpret_cast<float4*>(p) = v;
        else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
    };
    const bool live = t < T && t < feat_frames(frames, b, T);        // wave-uniform
    if (!live) {
        if (t < T && lane == 0) {
            dwork[(size_t)b * T + t] = 0.f;
            if (dist) dist[(size_t)b * T + t] = 0.f;
        }
        if (dr)
            for (int c = lane * 4; c < H; c += 256) store4(dr + c, make_float4(0.f, 0.f, 0.f, 0.f));
        return;
    }
    const float* hr = h + ((size_t)b * h_rows + t) * H;
    const float* rr = ref + ((size_t)b * ref_rows + t) * H;
    float4 h4[4], r4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = lane * 4 + 256 * u;
        h4[u] = c < H ? load4(hr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        r4[u] = c < H ? load4(rr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double shh = 0.0, srr = 0.0, shr = 0.0;
    auto acc = [&](const float4& a, const float4& r) {
        const double ax = a.x, ay = a.y, az = a.z, aw = a.w, rx = r.x, ry = r.y, rz = r.z, rw = r.w;
        shh += (ax * ax + ay * ay) + (az * az + aw * aw);
        srr += (rx * rx + ry * ry) + (rz * rz + rw * rw);
        shr += (ax * rx + ay * ry) + (az * rz + aw * rw);
    };
#pragma unroll
    for (int u = 0; u < 4; ++u) acc(h4[u], r4[u]);                    // columns past the row are zeros
    for (int c = 1024 + lane * 4; c < H; c += 256) acc(load4(hr + c), load4(rr + c));
    shh = wave_sum(shh); srr = wave_sum(srr); shr = wave_sum(shr);
    const double nh = sqrt(shh), nr = sqrt(srr);
    const bool degenerate = !(nh > FEAT_EPS) || !(nr > FEAT_EPS);
    const double cs = degenerate ? 0.0 : shr / (nh * nr);
    if (lane == 0) {
        const float d = (float)(1.0 - cs);
        dwork[(size_t)b * T + t] = d;
        if (dist) dist[(size_t)b * T + t] = d;
    }
    if (!dr) return;
    // dh = cr * r + ch * h, evaluated in double and rounded once per element
    const double cr = degenerate ? 0.0 : -(double)grad_scale / (nr * nh);
    const double ch = degenerate ? 0.0 : (double)grad_scale * cs / (nh * nh);
    auto emit = [&](int c, const float4& a, const float4& r) {
        store4(dr + c, make_float4((float)(cr * r.x + ch * a.x), (float)(cr * r.y + ch * a.y), (float)(cr * r.z + ch * a.z),
                                   (float)(cr * r.w + ch * a.w)));
    };
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane * 4 + 256 * u < H) emit(lane * 4 + 256 * u, h4[u], r4[u]);
    for (int c = 1024 + lane * 4; c < H; c += 256) emit(c, load4(hr + c), load4(rr + c));
}

// One workgroup per clip: thread i sums d[b][i], d[b][i + 256], ... in double, then the 256 partials are added in a fixed tree.
__global__ __launch_bounds__(256) void k_feat_loss(const float* __restrict__ dwork, const int32_t* __restrict__ frames, int T,
                                                   float* __restrict__ loss) {
    __shared__ double sm[256];
    const int b = blockIdx.x;
    const int Tb = feat_frames(frames, b, T);
    double s = 0.0;
    for (int t = threadIdx.x; t < Tb; t += 256) s += (double)dwork[(size_t)b * T + t];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[b] = (float)sm[0];
}

}  // namespace

int64_t feature_cos_work_floats(int B, int T) {
    if (B < 1 || T < 1) return 0;
    return ((int64_t)B * T + 3) / 4 * 4;
}

paa_status feature_cos(const float* h, int h_rows, const float* ref, int ref_rows, const int32_t* frames, int B, int T, int H,
                       float grad_scale, float* loss, float* dist, float* dh, float* work, hipStream_t st) {
    if (!h || !ref || !loss || !work) PAA_FAIL(PAA_ERR_ARG, "paa_feature_cos: null argument");
    if ((uintptr_t)work & 15) PAA_FAIL(PAA_ERR_ARG, "paa_feature_cos: the work buffer must be 16-byte aligned");
    if (B < 1 || T < 1 || h_rows < T || ref_rows < T)
        PAA_FAIL(PAA_ERR_SIZE, "paa_feature_cos: B=%d T=%d h_rows=%d ref_rows=%d (need B, T >= 1 and both row counts >= T)", B, T, h_rows,
                 ref_rows);
    if (H < 4 || H > 4096 || (H & 3)) PAA_FAIL(PAA_ERR_SIZE, "paa_feature_cos: H=%d must be a multiple of 4 in [4, 4096]", H);
    const int rows_per_clip = dh ? h_rows : T;          // with a cotangent the pad rows are visited too: they are written as zeros
    const int64_t rows = (int64_t)B * rows_per_clip;
    if (rows > ((int64_t)1 << 32)) PAA_FAIL(PAA_ERR_SIZE, "paa_feature_cos: %lld rows", (long long)rows);
    const bool vec = !(((uintptr_t)h | (uintptr_t)ref | (uintptr_t)dh) & 15);
    if (vec)
        hipLaunchKernelGGL(k_feat_cos<true>, dim3(cdiv(rows, 4)), dim3(256), 0, st, h, h_rows, ref, ref_rows, frames, B, T, H, grad_scale,
                           work, dist, dh, rows_per_clip);
    else
        hipLaunchKernelGGL(k_feat_cos<false>, dim3(cdiv(rows, 4)), dim3(256), 0, st, h, h_rows, ref, ref_rows, frames, B, T, H, grad_scale,
                           work, dist, dh, rows_per_clip);
    PAA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_feat_loss, dim3(B), dim3(256), 0, st, (const float*)work, frames, T, loss);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

}  // namespace paa

extern "C" int64_t paa_feature_cos_work_floats(int B, int T) { return paa::feature_cos_work_floats(B, T); }

extern "C" paa_status paa_feature_cos(const float* h, int h_rows, const float* ref, int ref_rows, const int32_t* d_frames, int B, int T,
                                      int H, float grad_scale, float* loss, float* dist, float* dh, float* work, void* stream) {
    return paa::feature_cos(h, h_rows, ref, ref_rows, d_frames, B, T, H, grad_scale, loss, dist, dh, work, (hipStream_t)stream);
}
