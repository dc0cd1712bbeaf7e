// mgrit_hip_transfer2d.inc -- spatial transfers between two Heat2D levels (MGRIT_HIP_TRANSFER_HEAT2D: grids with their rim,
// fine size 2 n_c - 1 per axis) and between two levels of one periodic application (MGRIT_HIP_TRANSFER_PERIODIC2D: Allen-Cahn,
// Cahn-Hilliard, Navier-Stokes, Gray-Scott, Burgers, Ginzburg-Landau; fine size 2 n_c per axis).
//
// The arithmetic is DESIGN.md 3.10, which is GridTransferHeat2D / GridTransferAllenCahn (pymgrit_amd/heat/grid_transfer_heat_2d.py,
// pymgrit_amd/allen_cahn/grid_transfer_allen_cahn.py) operand by operand: every sum left to right, no FMA (the file is built with
// -ffp-contract=off), the factors 4, 2, 1/2, 1/4 and 1/16 exact. The reference has no 2-D transfer class (core/grid_transfer.py:31-55
// is an open interface).
//
// A row holds q.planes planes one behind the other (Gray-Scott and Burgers: [u plane | v plane], GridTransferGrayScott /
// GridTransferBurgers; every other kind: one), a fine plane nxf * nyf values and a coarse one nxc * nyc. Plane c of the destination is
// the transfer of plane c of the source and of nothing else: no index of one plane, wrapped or not, reaches into the other.
//
// Launch shape of restrict2d_rows_kernel / interp2d_rows_kernel: blockIdx.x = pair, blockIdx.y = a tile of 256 consecutive positions
// of the DESTINATION row (its planes in their order, each in natural row-major order, x slow), one value per thread -- a tile may
// hold the end of one plane and the start of the next. Bandwidth-bound: consecutive threads walk along j, so
// the three fine rows a restriction tile reads are each one contiguous span whose cache lines are used whole between the
// terms j - 1, j, j + 1 (HBM sees every fine value once; the other terms come out of L1 / L2), and an interpolation tile reads
// two contiguous spans of half its own length.

struct T2DGeom { int nxf, nyf, nxc, nyc, periodic, planes; };

// dst row d_idx[p] <- R(src row s_idx[p]); positions behind the planes * nxc * nyc values (row pads) are written as zero
__global__ void restrict2d_rows_kernel(const double *__restrict__ src, int src_ld, const int32_t *__restrict__ s_idx,
                                       double *__restrict__ dst, int dst_ld, const int32_t *__restrict__ d_idx, T2DGeom q) {
    const int p = blockIdx.x, pos = blockIdx.y * blockDim.x + threadIdx.x;
    if (pos >= dst_ld) return;
    const double *f = src + (size_t)s_idx[p] * src_ld;
    double *c = dst + (size_t)d_idx[p] * dst_ld;
    const int nc = q.nxc * q.nyc;
    double r = 0.0;
    if (pos < q.planes * nc) {
        int pl = 0, rem = pos;   // the plane and the position in it (a step per plane in front: no division more than one plane needs)
        for (; pl + 1 < q.planes && rem >= nc; ++pl) rem -= nc;
        f += (size_t)pl * q.nxf * q.nyf;
        const int I = rem / q.nyc, J = rem - I * q.nyc, i = 2 * I, j = 2 * J;
        if (!q.periodic && (I == 0 || J == 0 || I == q.nxc - 1 || J == q.nyc - 1)) {
            r = f[(size_t)i * q.nyf + j];   // the rim by injection
        } else {
            // interior of a grid with its rim: 1 <= i - 1, i + 1 <= nxf - 2; periodic: i, j even and <= n - 2, only i - 1, j - 1 wrap
            const int im = i > 0 ? i - 1 : q.nxf - 1, jm = j > 0 ? j - 1 : q.nyf - 1, jp = j + 1;
            const double *fm = f + (size_t)im * q.nyf, *f0 = f + (size_t)i * q.nyf, *fp = f + (size_t)(i + 1) * q.nyf;
            r = (((((4.0 * f0[j] + 2.0 * (((fm[j] + fp[j]) + f0[jm]) + f0[jp])) + fm[jm]) + fm[jp]) + fp[jm]) + fp[jp]) / 16.0;
        }
    }
    c[pos] = r;
}

// mode 0: u^l_i = P(u^{l+1}_j)  (mgrit.py:562-563);  mode 1: u^l_i = u^l_i + P(u^{l+1}_j - v^{l+1}_j)  (mgrit.py:724-726);
// rows_out (mode 1): the corrected row goes to rows_out[p] instead of back into u^l (mgrit_hip_error_correction_to).
// Row pads (behind the planes * nxf * nyf values) are not touched: they stay zero.
__global__ void interp2d_rows_kernel(double *__restrict__ uf, int f_ld, const int32_t *__restrict__ f_idx,
                                     const double *__restrict__ uc, const double *__restrict__ vc, int c_ld,
                                     const int32_t *__restrict__ c_idx, T2DGeom q, int mode, double *__restrict__ rows_out, int ld_out) {
    const int p = blockIdx.x, pos = blockIdx.y * blockDim.x + threadIdx.x;
    const int nf = q.nxf * q.nyf;
    if (pos >= q.planes * nf) return;
    int pl = 0, rem = pos;   // the plane and the position in it (a step per plane in front: no division more than one plane needs)
    for (; pl + 1 < q.planes && rem >= nf; ++pl) rem -= nf;
    double *f = uf + (size_t)f_idx[p] * f_ld;
    const size_t c_off = (size_t)c_idx[p] * c_ld + (size_t)pl * q.nxc * q.nyc;
    const double *e = uc + c_off;
    const double *e2 = mode == 1 ? vc + c_off : nullptr;
    const int i = rem / q.nyf, j = rem - i * q.nyf, I = i >> 1, J = j >> 1;
    // a grid with its rim: an odd i has I + 1 <= nxc - 1; periodic: I + 1 = nxc wraps to 0 (only reached for odd i / odd j)
    const int I1 = I + 1 < q.nxc ? I + 1 : 0, J1 = J + 1 < q.nyc ? J + 1 : 0;
    auto at = [&](int a, int b) { const size_t k = (size_t)a * q.nyc + b; return e2 ? e[k] - e2[k] : e[k]; };
    double val;
    if (!(i & 1) && !(j & 1)) val = at(I, J);
    else if (!(j & 1)) val = (at(I, J) + at(I1, J)) / 2.0;
    else if (!(i & 1)) val = (at(I, J) + at(I, J1)) / 2.0;
    else val = (((at(I, J) + at(I1, J)) + at(I, J1)) + at(I1, J1)) / 4.0;
    if (rows_out) rows_out[(size_t)p * ld_out + pos] = f[pos] + val;
    else f[pos] = mode == 0 ? val : f[pos] + val;
}
