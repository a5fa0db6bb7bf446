// Box-snippet harvest on gfx950: the points of a sweep inside a tracked box, in box coordinates, for many (sweep, box) jobs per
// call.  C ABI and semantics: include/liso_snippets.h.  Compiled without FMA contraction: every expression is the header's,
// operation by operation.
//
// prep  : one thread per job -- inverse pose and fp32 half extents, and the job's rank in a stable order by sweep, so that the
//         jobs of one sweep are one run [lo, hi) of the sorted table (jobs with no sweep sort behind every sweep).
// count : one block = 256 consecutive rows of one sweep, read once, against the sweep's jobs staged in LDS 32 at a time; per job
//         one ballot per wave; the block's count goes to counts[rank][chunk].
// scan  : per job an exclusive scan over its chunks (in place), then one block scans the job totals into out_offsets (int64).
// move  : the count pass again; a point's position is offsets[job] + chunk prefix + popcount of the ballots in front of its lane.
//         Only rows below `capacity` are written.
// The work is bound by reading the sweeps (twice) and by the launch count (five), not by arithmetic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_snippets.h"
#include "dev_common.h"

namespace {

using liso_dev::Carver;
using liso_dev::check_launch;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 32;  // jobs staged in LDS at a time

struct JobRow {
    double m[12];  // rows x, y, z of box_T_sensor
    float h[3];    // 0.55f * dims
    int job;       // index of the job in the caller's order
};


struct Tables {
    JobRow* rows;     // [J] in sorted order
    int32_t* key;     // [J] sweep of the sorted job, n_clouds for none
    int32_t* total;   // [J] points of job j (caller's order)
    int32_t* counts;  // [J][chunks] per sorted job and chunk: count, then the exclusive prefix over the chunks
    size_t bytes;
};

Tables carve(int J, int chunks, void* base) {
    Tables t;
    Carver ws{base};
    t.rows = ws.take<JobRow>((size_t)J);
    t.key = ws.take<int32_t>((size_t)J);
    t.total = ws.take<int32_t>((size_t)J);
    t.counts = ws.take<int32_t>((size_t)J * chunks);
    t.bytes = ws.bytes;
    return t;
}

__device__ __forceinline__ int key_of(int cloud, int T) { return (cloud >= 0 && cloud < T) ? cloud : T; }

__global__ __launch_bounds__(kThreads) void prep_kernel(int T, int J, const int32_t* job_cloud, const float* boxes, Tables t,
                                                        double* out_box_T_sensor) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= J) return;
    const int key = key_of(job_cloud[j], T);
    int rank = 0;
    for (int o = 0; o < J; ++o) {
        const int ko = key_of(job_cloud[o], T);
        rank += (ko < key || (ko == key && o < j)) ? 1 : 0;
    }
    const float* b = boxes + (size_t)j * 7;
    const double x = b[0], y = b[1], z = b[2], yaw = b[6];
    const double c = cos(yaw), s = sin(yaw);
    JobRow r;
    r.m[0] = c, r.m[1] = s, r.m[2] = 0.0, r.m[3] = -(c * x + s * y);
    r.m[4] = -s, r.m[5] = c, r.m[6] = 0.0, r.m[7] = s * x - c * y;
    r.m[8] = 0.0, r.m[9] = 0.0, r.m[10] = 1.0, r.m[11] = -z;
    for (int a = 0; a < 3; ++a) r.h[a] = 0.55f * b[3 + a];
    r.job = j;
    t.rows[rank] = r;
    t.key[rank] = key;
    if (out_box_T_sensor) {
        double* o = out_box_T_sensor + (size_t)j * 16;
        for (int a = 0; a < 12; ++a) o[a] = r.m[a];
        o[12] = 0.0, o[13] = 0.0, o[14] = 0.0, o[15] = 1.0;
    }
}

// first sorted job whose key is >= k
__device__ int lower_bound(const int32_t* key, int J, int k) {
    int lo = 0, hi = J;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (key[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool inside(const JobRow& r, double x, double y, double z, float* q) {
    bool in = true;
    for (int a = 0; a < 3; ++a) {
        q[a] = (float)(((r.m[4 * a] * x + r.m[4 * a + 1] * y) + r.m[4 * a + 2] * z) + r.m[4 * a + 3]);
        in = in && fabsf(q[a]) <= r.h[a];
    }
    return in;
}

// MOVE == false: counts[rank][chunk] <- points of the chunk inside the job's box.
// MOVE == true : counts holds the exclusive prefix over the chunks; the points are written.
template <bool MOVE>
__global__ __launch_bounds__(kThreads) void cut_kernel(int N, int stride, int J, int chunks, const float* clouds, const int32_t* counts_in,
                                                       const int32_t* lidar_rows, Tables t, long capacity, const int64_t* offsets,
                                                       float* out_points, int32_t* out_rows) {
    __shared__ JobRow rows[kTile];
    __shared__ unsigned long long ballots[kTile][kWaves];
    __shared__ int range[2];
    const int cloud = blockIdx.y, chunk = blockIdx.x;
    if (threadIdx.x == 0) range[0] = lower_bound(t.key, J, cloud), range[1] = lower_bound(t.key, J, cloud + 1);
    __syncthreads();
    const int lo = range[0], hi = range[1];
    if (lo == hi) return;  // no job names this sweep: nothing of it is read
    int n = N;
    if (counts_in) n = counts_in[cloud], n = n < 0 ? 0 : (n > N ? N : n);
    const int i = chunk * kThreads + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row = (size_t)cloud * N + i;
    bool valid = i < n;
    double x = 0.0, y = 0.0, z = 0.0;
    float intensity = 0.f;
    if (valid) {
        const float* p = clouds + row * stride;
        const float xf = p[0], yf = p[1], zf = p[2];
        valid = !(isnan(xf) || isnan(yf) || isnan(zf));
        x = xf, y = yf, z = zf;
        if (MOVE) intensity = p[stride - 1];
    }
    for (int k0 = lo; k0 < hi; k0 += kTile) {
        const int tk = min(kTile, hi - k0);
        __syncthreads();  // the previous tile is done with rows / ballots
        for (int w = threadIdx.x; w < tk * (int)(sizeof(JobRow) / 4); w += kThreads) ((uint32_t*)rows)[w] = ((const uint32_t*)(t.rows + k0))[w];
        __syncthreads();
        uint32_t mine = 0;  // jobs of the tile that hold this thread's point
        for (int k = 0; k < tk; ++k) {
            float q[3];
            const bool in = valid && inside(rows[k], x, y, z, q);
            const unsigned long long bal = __ballot(in);
            if (lane == 0) ballots[k][wave] = bal;
            mine |= (uint32_t)in << k;
        }
        __syncthreads();
        if (!MOVE) {
            if ((int)threadIdx.x < tk) {
                int c = 0;
                for (int w = 0; w < kWaves; ++w) c += __popcll(ballots[threadIdx.x][w]);
                t.counts[(size_t)(k0 + threadIdx.x) * chunks + chunk] = c;
            }
            continue;
        }
        while (mine) {
            const int k = __ffs(mine) - 1;
            mine &= mine - 1;
            int before = __popcll(ballots[k][wave] & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) before += __popcll(ballots[k][w]);
            const long to = (long)offsets[rows[k].job] + t.counts[(size_t)(k0 + k) * chunks + chunk] + before;
            if (to < capacity) {
                float q[3];
                inside(rows[k], x, y, z, q);
                *(float4*)(out_points + (size_t)to * 4) = make_float4(q[0], q[1], q[2], intensity);
                if (out_rows) out_rows[to] = lidar_rows[row];
            }
        }
    }
}

// one block per sorted job: counts[rank][:] <- its exclusive prefix, total[job] <- the sum (0 for a job without a sweep)
__global__ __launch_bounds__(kThreads) void scan_chunks_kernel(int T, int chunks, Tables t) {
    __shared__ int part[kThreads];
    const int r = blockIdx.x, job = t.rows[r].job;
    if (t.key[r] >= T || chunks == 0) {
        if (threadIdx.x == 0) t.total[job] = 0;
        return;
    }
    int32_t* c = t.counts + (size_t)r * chunks;
    const int per = (chunks + kThreads - 1) / kThreads, a0 = min(chunks, (int)threadIdx.x * per), a1 = min(chunks, a0 + per);
    int sum = 0;
    for (int a = a0; a < a1; ++a) sum += c[a];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < kThreads; ++w) {
            const int v = part[w];
            part[w] = run;
            run += v;
        }
        t.total[job] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int a = a0; a < a1; ++a) {
        const int v = c[a];
        c[a] = run;
        run += v;
    }
}

// one block: out_offsets <- exclusive prefix of total (int64), J + 1 entries
__global__ __launch_bounds__(kThreads) void scan_jobs_kernel(int J, const int32_t* total, int64_t* out_offsets) {
    __shared__ long long part[kThreads];
    const int per = (J + kThreads - 1) / kThreads, a0 = min(J, (int)threadIdx.x * per), a1 = min(J, a0 + per);
    long long sum = 0;
    for (int a = a0; a < a1; ++a) sum += total[a];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int w = 0; w < kThreads; ++w) {
            const long long v = part[w];
            part[w] = run;
            run += v;
        }
        out_offsets[J] = run;
    }
    __syncthreads();
    long long run = part[threadIdx.x];
    for (int a = a0; a < a1; ++a) {
        out_offsets[a] = run;
        run += total[a];
    }
}

int chunks_of(int n_max) { return (n_max + kThreads - 1) / kThreads; }

bool sizes_ok(int T, int N, int J) {
    return T >= 0 && T <= LISO_SNIPPET_MAX_CLOUDS && N >= 0 && N <= LISO_SNIPPET_MAX_N && J >= 0 && J <= LISO_SNIPPET_MAX_JOBS;
}

}  // namespace

extern "C" {

size_t liso_snippet_cut_workspace_bytes(int n_clouds, int n_max, int n_jobs) {
    if (!sizes_ok(n_clouds, n_max, n_jobs)) return 0;
    return carve(n_jobs, chunks_of(n_max), nullptr).bytes + 256;  // never 0 for valid sizes
}

int liso_snippet_cut_f32(int n_clouds, int n_max, int point_stride, const float* clouds, const int32_t* counts,
                         const int32_t* lidar_rows, int n_jobs, const int32_t* job_cloud, const float* job_boxes, long capacity,
                         int64_t* out_offsets, float* out_points, int32_t* out_rows, double* out_box_T_sensor, void* workspace,
                         size_t workspace_bytes, void* stream) {
    const int T = n_clouds, N = n_max, J = n_jobs;
    if (!sizes_ok(T, N, J) || point_stride < 4 || capacity < 0 || !out_offsets) return LISO_EINVAL;
    if (T > 0 && N > 0 && !clouds) return LISO_EINVAL;
    if ((lidar_rows == nullptr) != (out_rows == nullptr)) return LISO_EINVAL;
    if (capacity > 0 && !out_points) return LISO_EINVAL;
    if (J > 0 && (!job_cloud || !job_boxes)) return LISO_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 7) != 0) return LISO_EINVAL;
    if (((uintptr_t)out_points & 15) != 0) return LISO_EINVAL;  // rows are written as one 16-byte store
    const int chunks = chunks_of(N);
    const Tables t = carve(J, chunks, workspace);
    if (workspace_bytes < t.bytes + 256) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const bool sweep = J > 0 && T > 0 && chunks > 0;
    if (J > 0) {
        prep_kernel<<<(J + kThreads - 1) / kThreads, kThreads, 0, st>>>(T, J, job_cloud, job_boxes, t, out_box_T_sensor);
        if (sweep)
            cut_kernel<false><<<dim3(chunks, T), kThreads, 0, st>>>(N, point_stride, J, chunks, clouds, counts, lidar_rows, t, 0, nullptr,
                                                                    nullptr, nullptr);
        scan_chunks_kernel<<<J, kThreads, 0, st>>>(T, sweep ? chunks : 0, t);
    }
    scan_jobs_kernel<<<1, kThreads, 0, st>>>(J, t.total, out_offsets);
    if (sweep && capacity > 0)
        cut_kernel<true><<<dim3(chunks, T), kThreads, 0, st>>>(N, point_stride, J, chunks, clouds, counts, lidar_rows, t, capacity,
                                                               out_offsets, out_points, out_rows);
    return check_launch();
}

}  // extern "C"
