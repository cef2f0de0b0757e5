// tb_mech_gather.hip — ElementAssemblyStrategy on three-component hexahedral fields, second pass: the stored element matrices Kₑ / residuals rₑ
// of tb_mechanics.hip and tb_mech_split.hip are summed into the CSR rows / the residual, every sum in cell order (bit-reproducible like the
// reference's EA strategy).  The host planning is tb::plan::node_list / node_row_check / gather_nodes (tb_planners.cpp); here are the kernels,
// their launchers and the upload tails.
#include <hip/hip_runtime.h>

#include "tb_internal.h"
#include "tb_mech_common.hpp"
#include "tb_mech_gather.hpp"

namespace tb {
using namespace tbk;

// Direct gather, one wave per node.  A lane owns *positions* of the node's three CSR rows, not source entries: per cell touching the node a byte
// map "neighbour-node slot of the row → local node b" is built in LDS from blockpos (27 byte stores), then every lane sums its entry over the
// ≤8 element matrices in cell order — independent loads, all in flight together, no accumulator in LDS, each nz stored once.
// TL: the element matrices are stored in tensor order (tb_mech_common.hpp) instead of Ferrite's.
template <int NB, int NK, bool TL>
__device__ __forceinline__ void gather_rows(const double *const (&rowk)[8], const uint8_t *inv, int nbr_max, int L, int lane, double *dst0, bool first)
{
    // the three rows of the node share the position → local-node lookup: one pass over the positions with the 3·NK loads of a position in flight
    // together (constant offsets c·ND from one address), instead of three passes of NK loads each
    constexpr int ND = 3 * NB;
    for (int p = lane; p < L; p += 64) {
        const int nbr = p / 3, d = p - 3 * nbr;
        double v[3][NK];
        bool ok[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int b = inv[k * nbr_max + nbr];
            ok[k] = b != 0xFF;
            const int bb = ok[k] ? b : 0;
            const double *src = rowk[k] + (TL ? bb + 9 * d : 3 * bb + d); // TL: the map holds cb(b) (tensor-order columns)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][k] = src[c * ND];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < NK; ++k) sum += ok[k] ? v[c][k] : 0.0;
            double *dst = dst0 + (int64_t)c * L;
            if (first) dst[p] = sum; else dst[p] += sum;
        }
    }
}

// The fall-back of the staged gather below: meshes where a node sits in more than 8 cells or a node row holds more than 384 positions.  Bound by
// its chain of dependent trips (12.8 ms against 9.1 ms at 80³).
template <int NB, bool TL>
__global__ void __launch_bounds__(256)
k_gather_node_rows(const int32_t *__restrict__ node_dof0, int64_t n_nodes, const int64_t *__restrict__ ea_ptr, const int32_t *__restrict__ ea_src,
                   const double *__restrict__ ke, const uint16_t *__restrict__ blockpos, const int64_t *__restrict__ rowptr, double *__restrict__ nz,
                   int nbr_max)
{
    constexpr int ND = 3 * NB, KC = 8;
    extern __shared__ uint8_t s_inv[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t node = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    if (node >= n_nodes) return;
    uint8_t *inv = s_inv + (size_t)wv * KC * nbr_max;
    const int32_t dof0 = node_dof0[node];
    const int64_t g0 = rowptr[dof0];
    const int L = (int)(rowptr[dof0 + 1] - g0); // rows dof0, dof0+1, dof0+2 are consecutive runs of equal length (checked on the host)
    const int64_t k0 = ea_ptr[dof0], k1 = ea_ptr[dof0 + 1];
    for (int64_t kb = k0; kb < k1; kb += KC) {
        const int nk = (int)(k1 - kb < KC ? k1 - kb : KC);
        const int nkp = nk <= 2 ? nk : nk <= 4 ? 4 : 8; // padded slots repeat cell 0 with an all-0xFF map: contribute nothing
        for (int i = lane; i < nkp * nbr_max / 4; i += 64) reinterpret_cast<uint32_t *>(inv)[i] = 0xFFFFFFFFu;
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < nk * NB; i += 64) {
            const int k = i / NB, b = i - k * NB;
            const int32_t slot = ea_src[kb + k];
            const int64_t cell = slot / ND;
            const int a = (slot % ND) / 3;
            inv[k * nbr_max + blockpos[cell * (NB * NB) + a * NB + b] / 3] = (uint8_t)(TL ? cb27(b) : b);
        }
        __builtin_amdgcn_wave_barrier();
        const double *rowk[8];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int32_t slot = ea_src[kb + (k < nk ? k : 0)];
            rowk[k] = ke + ((int64_t)(slot / ND) * ND + 3 * (TL ? tix27((slot % ND) / 3) : (slot % ND) / 3)) * ND;
        }
        const bool first = kb == k0;
        if (nkp == 1) gather_rows<NB, 1, TL>(rowk, inv, nbr_max, L, lane, nz + g0, first);
        else if (nkp == 2) gather_rows<NB, 2, TL>(rowk, inv, nbr_max, L, lane, nz + g0, first);
        else if (nkp == 4) gather_rows<NB, 4, TL>(rowk, inv, nbr_max, L, lane, nz + g0, first);
        else gather_rows<NB, 8, TL>(rowk, inv, nbr_max, L, lane, nz + g0, first);
        __builtin_amdgcn_wave_barrier();
    }
}

// The same gather with the source rows staged through LDS and the per-node metadata in one record (default when a node's rows hold ≤ 384 positions
// and no node sits in more than 8 cells).  The kernel above is bound by its chain of dependent trips (dof → row pointers and slot range → slots →
// block positions → data, then one trip per 64 positions of each row): ≈ 19 µs per node with 24 waves per CU.  Here a wave reads ONE 48-byte record
// (GatherNode, tb_planners.hpp), then — in the same trip — the block positions of its cells and the cells' runs themselves (a node's share of an
// element matrix is one contiguous run, rows 3a..3a+2 of Kₑ: 3·ND doubles, read coalesced, every line once), parks both in LDS and sums from LDS
// into registers: a lane owns positions lane + 64·i of the three rows, contributions added in cell order (bit-reproducible); every nz stored once,
// coalesced.  TL: rows / columns of the stored element matrices in tensor order (tb_mech_common.hpp) instead of Ferrite's.
template <int NB, int KC, bool TL>
__global__ void __launch_bounds__(256, KC == 4 ? 4 : 2)
k_gather_node_rows_lds(const GatherNode *__restrict__ gn, int64_t n_nodes, const double *__restrict__ ke, const uint16_t *__restrict__ blockpos,
                       double *__restrict__ nz, int nbr_pad)
{
    constexpr int ND = 3 * NB, RUN = 3 * ND, NJ = (RUN + 63) / 64, NI = 6;
    extern __shared__ double s_stage[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)blockIdx.x * 4 + wv;
    if (node >= n_nodes) return; // no workgroup barrier below: waves are independent
    double *buf = s_stage + (size_t)wv * (KC * RUN + KC * nbr_pad / 8);
    uint8_t *inv = reinterpret_cast<uint8_t *>(buf + KC * RUN);
    const GatherNode rec = gn[node];
    const int L = rec.L;
    double acc[NI][3];
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0;
#pragma unroll
    for (int kb = 0; kb < 8; kb += KC) {
        if (kb >= rec.nk) break;
        const int nk = rec.nk - kb < KC ? rec.nk - kb : KC;
        double r[KC][NJ];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (k < nk) {
                int64_t row0 = rec.slot[kb + k]; // cell·ND + 3a
                if constexpr (TL) { const int64_t cellk = row0 / ND; row0 = cellk * ND + 3 * tix27((int)(row0 - cellk * ND) / 3); }
                const double *src = ke + row0 * ND;
#pragma unroll
                for (int j = 0; j < NJ; ++j) { const int idx = lane + 64 * j; r[k][j] = idx < RUN ? src[idx] : 0.0; }
            }
        }
        for (int i = lane; i < nk * nbr_pad / 4; i += 64) reinterpret_cast<uint32_t *>(inv)[i] = 0xFFFFFFFFu;
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < nk * NB; i += 64) {
            const int k = i / NB, b = i - k * NB;
            int32_t slot = rec.slot[kb];
#pragma unroll
            for (int kk = 1; kk < KC; ++kk) slot = k == kk ? rec.slot[kb + kk] : slot;
            const int64_t cell = slot / ND;
            const int a = (slot - (int32_t)cell * ND) / 3;
            inv[k * nbr_pad + blockpos[cell * (NB * NB) + a * NB + b] / 3] = (uint8_t)(TL ? cb27(b) : b);
        }
#pragma unroll
        for (int k = 0; k < KC; ++k)
            if (k < nk) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) { const int idx = lane + 64 * j; if (idx < RUN) buf[k * RUN + idx] = r[k][j]; }
            }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int p = lane + 64 * i;
            if (p < L) {
                const int nbr = p / 3, d = p - 3 * nbr;
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (k < nk) {
                        const int b = inv[k * nbr_pad + nbr];
                        if (b != 0xFF) {
                            const double *sv = buf + k * RUN + (TL ? b + 9 * d : 3 * b + d);
                            acc[i][0] += sv[0];
                            acc[i][1] += sv[ND];
                            acc[i][2] += sv[2 * ND];
                        }
                    }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = lane + 64 * i;
        if (p < L) {
            nz[rec.g0 + p] = acc[i][0];
            nz[rec.g0 + L + p] = acc[i][1];
            nz[rec.g0 + 2 * (int64_t)L + p] = acc[i][2];
        }
    }
}

// element residuals → global residual: r[d] = Σ (in cell order) rₑ slots of dof d
__global__ void k_gather_residual(const int64_t *__restrict__ ptr, const int32_t *__restrict__ src, const double *__restrict__ re, int64_t ndofs,
                                  double *__restrict__ r)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= ndofs) return;
    double s = 0.0;
    for (int64_t k = ptr[d]; k < ptr[d + 1]; ++k) s += re[src[k]];
    r[d] = s;
}

// ------------------------------------------------------------------------------------------------ host side
static plan::MeshView view(const tb_mesh *m) { return {m->n_nodes, m->n_cells, m->ndofs, m->nverts, 3 * m->nb, 3, m->h_xyz.data(), m->h_conn.data(), m->h_cell_dofs.data()}; }
static plan::PatternView view(const tb_pattern *p) { return {p->n_rows, p->h_rowptr.data(), p->h_colidx.data(), p->max_row_len}; }

int prepare_tangent_gather(tb_pattern *p)
{
    tb_mesh *m = p->mesh;
    if (!m->d_node_dof0) {
        m->h_node_dof0 = plan::node_list(view(m));
        m->n_nodes_field = (int64_t)m->h_node_dof0.size();
        TB_TRY(upload(m->dev, m->h_node_dof0, &m->d_node_dof0));
    }
    if (!p->max_row_len) {
        int64_t L = 0;
        const int rc = plan::node_row_check(view(p), m->h_node_dof0, L);
        if (rc) return rc;
        p->max_row_len = L;
    }
    if (p->gnodes_state) return TB_OK;
    TB_NO_CAPTURE(m->dev);
    const plan::GatherHost h = plan::gather_nodes(view(m), view(p), m->h_node_dof0);
    if (!h.applicable) { p->gnodes_state = -1; return TB_OK; }
    p->h_gn_last = h.last;
    TB_HIP(hipMalloc(&p->d_gnodes, sizeof(GatherNode) * h.recs.size()));
    TB_HIP(hipMemcpy(p->d_gnodes, h.recs.data(), sizeof(GatherNode) * h.recs.size(), hipMemcpyHostToDevice));
    p->gnodes_state = 1;
    return TB_OK;
}

int launch_tangent_gather(tb_pattern *p, hipStream_t stream, int64_t n0, int64_t n1, const double *d_ke, double *d_nz)
{
    const tb_mesh *m = p->mesh;
    const bool q2 = m->nb == 27; // the triquadratic field stores its element matrices in tensor order
    const int nbr_max = (((int)p->max_row_len / 3) + 3) & ~3;
    const dim3 grid((unsigned)((n1 - n0 + 3) / 4));
    if (p->gnodes_state > 0) {
        const int nbr_pad = (nbr_max + 7) & ~7;
        const size_t lds = (size_t)4 * 4 * (3 * (3 * m->nb) * sizeof(double) + (size_t)nbr_pad);
        const GatherNode *gn = (const GatherNode *)p->d_gnodes + n0;
        if (q2) hipLaunchKernelGGL((k_gather_node_rows_lds<27, 4, true>), grid, dim3(256), lds, stream, gn, n1 - n0, d_ke, p->d_blockpos, d_nz, nbr_pad);
        else hipLaunchKernelGGL((k_gather_node_rows_lds<8, 4, false>), grid, dim3(256), lds, stream, gn, n1 - n0, d_ke, p->d_blockpos, d_nz, nbr_pad);
    } else {
        const size_t lds = (size_t)4 * 8 * nbr_max;
        if (q2) hipLaunchKernelGGL((k_gather_node_rows<27, true>), grid, dim3(256), lds, stream, m->d_node_dof0 + n0, n1 - n0, m->ea->d_ptr, m->ea->d_src, d_ke, p->d_blockpos, p->d_rowptr, d_nz, nbr_max);
        else hipLaunchKernelGGL((k_gather_node_rows<8, false>), grid, dim3(256), lds, stream, m->d_node_dof0 + n0, n1 - n0, m->ea->d_ptr, m->ea->d_src, d_ke, p->d_blockpos, p->d_rowptr, d_nz, nbr_max);
    }
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int launch_residual_gather(tb_mesh *m, const double *d_re, double *d_r)
{
    hipLaunchKernelGGL(k_gather_residual, dim3((unsigned)((m->ndofs + 255) / 256)), dim3(256), 0, m->dev->stream, m->ea->d_ptr, m->ea->d_src, d_re, m->ndofs, d_r);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

} // namespace tb
