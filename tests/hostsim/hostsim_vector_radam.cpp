// g++ build of the vector models' RiemannianAdam row (sympa_amd/csrc/vector_math.hpp) for the CPU tests:
// the per-lane sums, the xor butterfly over the G lanes of a row emulated with a loop, the scalar epilogues and the
// per-coordinate outputs, in the order vec_radam_kernel of sympa_amd/csrc/vector_models.hip runs them.  G = 0 takes the
// kernel's own choice (vec_lanes).
#include <cstdint>
#include <vector>

#include "../../sympa_amd/csrc/vector_math.hpp"

namespace {
using namespace sympa;

// v[l] <- v[l] + v[l ^ off], off = G / 2, ..., 1: what `v += __shfl_xor(v, off)` leaves in lane l
void butterfly(std::vector<double>& v) {
    const int G = (int)v.size();
    std::vector<double> w(G);
    for (int off = G / 2; off > 0; off >>= 1) {
        for (int l = 0; l < G; ++l) w[l] = v[l] + v[l ^ off];
        v = w;
    }
}

bool valid_lanes(int G) { return G == 1 || G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64; }

// one round: every lane accumulates its coordinates into a sums struct of its own (accumulate(i, sums)), then each listed
// member goes through the butterfly and lane 0's value is kept
template <typename Sums, typename Zero, typename Acc>
Sums lane_round(int dims, int G, Zero zero, Acc accumulate, std::vector<double (Sums::*)[VEC_MAX_FACTORS]> members) {
    std::vector<Sums> lanes(G);
    for (int l = 0; l < G; ++l) {
        zero(lanes[l]);
        for (int i = 2 * l; i < dims; i += 2 * G)
            for (int k = 0; k < 2 && i + k < dims; ++k) accumulate(i + k, lanes[l]);
    }
    Sums out = lanes[0];
    for (auto mem : members)
        for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
            std::vector<double> v(G);
            for (int l = 0; l < G; ++l) v[l] = (lanes[l].*mem)[f];
            butterfly(v);
            (out.*mem)[f] = v[0];
        }
    return out;
}

struct RestSums {
    double rest[VEC_MAX_FACTORS];
};
}  // namespace

extern "C" {

// x, m, s [b, dims] are updated in place, like the kernel's table, exp_avg and exp_avg_sq.  p1, p2: beta^t of this step.
// moved_rows: rows whose Poincare factor was projected; status: the or of the rows' status bits.
int sympa_hostsim_vector_radam(double* x, const double* g, double* m, double* s, int64_t b, int dims, int model, int G, double lr,
                               double beta1, double beta2, double eps_adam, double wd, double coef, double p1, double p2,
                               int32_t* moved_rows, int32_t* status) {
    VecLayout L;
    if (!vec_layout(model, dims, L)) return -1;
    if (G == 0) G = vec_lanes(dims);
    if (!valid_lanes(G)) return -1;
    VecAdamParams P;
    P.lr = lr; P.beta1 = beta1; P.beta2 = beta2; P.eps = eps_adam; P.wd = wd; P.coef = coef;
    P.bc1 = 1.0 - p1;
    P.bc2 = 1.0 - p2;
    bool has_l = false;
    for (int f = 0; f < L.nf; ++f) has_l = has_l || L.geom[f] == VG_L;
    int moved_count = 0, st_all = 0;
    std::vector<double> yo(dims), mo(dims), so(dims);
    for (int64_t p = 0; p < b; ++p) {
        double* xp = x + p * dims;
        const double* gp = g + p * dims;
        double* mp = m + p * dims;
        double* sp = s + p * dims;
        // round 1
        const VecRowSums rs = lane_round<VecRowSums>(
            dims, G, [](VecRowSums& t) { vec_row_sums_zero(t); },
            [&](int i, VecRowSums& t) { vec_row_accumulate(L, i, xp[i], vec_row_grad(gp[i], xp[i], P.coef, P.wd), t); },
            {&VecRowSums::xx, &VecRowSums::xg});
        int st = vec_row_status(L, rs);
        auto coord = [&](int i) {
            VecAdamCoord c;
            vec_adam_coord(L, rs, P, i, xp[i], gp[i], mp[i], sp[i], c);
            return c;
        };
        // round 2
        const VecAdamSums S = lane_round<VecAdamSums>(
            dims, G, [](VecAdamSums& t) { vec_adam_sums_zero(t); },
            [&](int i, VecAdamSums& t) { vec_adam_accumulate(L, i, coord(i), t); },
            {&VecAdamSums::rr, &VecAdamSums::xm, &VecAdamSums::mm, &VecAdamSums::sin});
        VecAdamStep as;
        double ww[VEC_MAX_FACTORS];
        vec_adam_step(L, rs, S, P, as, ww);
        bool moved = false;
        VecRowStep sc;
        vec_row_step_coef(L, ww, sc, moved);
        auto stage2 = [&](int i, const VecAdamCoord& c) { return vec_row_stage2(L, sc, i, c.x, vec_adam_stage1(L, as, P, i, c)); };
        // round 3
        double rest[VEC_MAX_FACTORS] = {0.0, 0.0};
        if (has_l) {
            const RestSums r = lane_round<RestSums>(
                dims, G, [](RestSums& t) { t.rest[0] = 0.0; t.rest[1] = 0.0; },
                [&](int i, RestSums& t) {
                    const int f = vec_factor_of(L, i);
                    if (i == L.begin[f]) return;
                    const double z = stage2(i, coord(i));
                    t.rest[f] = d_fma(z, z, t.rest[f]);
                },
                {&RestSums::rest});
            rest[0] = r.rest[0]; rest[1] = r.rest[1];
        }
        // round 4
        const VecTranspSums T = lane_round<VecTranspSums>(
            dims, G, [](VecTranspSums& t) { vec_transp_sums_zero(t); },
            [&](int i, VecTranspSums& t) {
                const VecAdamCoord c = coord(i);
                vec_transp_accumulate(L, i, c.x, vec_row_final(L, rest, i, stage2(i, c)), c.m1, t);
            },
            {&VecTranspSums::ym, &VecTranspSums::xy, &VecTranspSums::yy});
        VecTransp tc;
        vec_transp_coef(L, rs.xx, S.xm, T, tc);
        st |= vec_adam_status(L, S, ww, T);
        for (int i = 0; i < dims; ++i) {
            const VecAdamCoord c = coord(i);
            yo[i] = vec_row_final(L, rest, i, stage2(i, c));
            mo[i] = vec_transp_coord(L, tc, i, c.x, yo[i], c.m1);
            so[i] = vec_adam_s1(L, as, P, i, c);
        }
        for (int i = 0; i < dims; ++i) { xp[i] = yo[i]; mp[i] = mo[i]; sp[i] = so[i]; }
        moved_count += moved ? 1 : 0;
        st_all |= st;
    }
    if (moved_rows != nullptr) *moved_rows = moved_count;
    if (status != nullptr) *status = st_all;
    return 0;
}

}  // extern "C"
