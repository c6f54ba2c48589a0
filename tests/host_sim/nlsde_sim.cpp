// CPU build of the arithmetic of the non-linear SDE kernels (markovflow_amd/csrc/mf_nlsde_math.hpp): a stand-alone program that
// runs the very functions em_kernel, linearize_kernel and drift_difference_kernel (mf_nlsde.hip) call per lane.  Plain host
// compilation with the system compiler, no HIP headers, nothing preloaded.  Test infrastructure (tests/test_sde_host.py).
//
//   nlsde_sim f64|f32 < commands        one result line per command, every number as a hexadecimal float (exact both ways)
//     rule nq x_0 .. x_{nq-1} w_0 .. w_{nq-1}        the Gauss-Hermite rule of the commands that follow (weights sum to sqrt pi)
//     em d drift p0 dt l_0 .. x_0 .. xi_0 ..         one Euler-Maruyama step: d (d + 1) / 2 entries of L, the state, the draw -> d numbers
//     lin drift p0 l m S dt                          one point of the linearisation -> A b cholQ
//     dd drift p0 m S A b scale                      one point of the drift difference -> val g_m g_S g_A g_b
// Exit status 0, or 2 on a malformed command.
#include "../../markovflow_amd/csrc/mf_nlsde_math.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace {
using namespace mf::nlsde;

bool read_numbers(std::istringstream& in, std::vector<double>& out) {
    std::string tok;
    while (in >> tok) {
        char* end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end != '\0') return false;
        out.push_back(v);
    }
    return true;
}

template <typename T> void print(const std::vector<T>& vals) {
    for (size_t i = 0; i < vals.size(); ++i) std::printf(i ? " %a" : "%a", double(vals[i]));
    std::printf("\n");
}

template <typename T, int D>
bool em_case(int drift, const std::vector<double>& v) {
    constexpr int TRI = D * (D + 1) / 2;
    if (v.size() != size_t(4 + TRI + 2 * D)) return false;
    Par<T> p{T(v[2])};
    Chol<T> L;
    for (int i = 0; i < MAX_D * (MAX_D + 1) / 2; ++i) L.l[i] = i < TRI ? T(v[4 + i]) : T(0);
    T x[D], xi[D];
    for (int i = 0; i < D; ++i) {
        x[i] = T(v[4 + TRI + i]);
        xi[i] = T(v[4 + TRI + D + i]);
    }
    const T dt = T(v[3]);
    if (drift == 0) em_step<T, D, 0>(x, xi, dt, t_sqrt(dt), L, p);
    else em_step<T, D, 1>(x, xi, dt, t_sqrt(dt), L, p);
    print(std::vector<T>(x, x + D));
    return true;
}

template <typename T>
int run() {
    Rule<T> q;
    q.nq = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::vector<double> v;
        if (!read_numbers(in, v)) return 2;
        if (cmd == "rule") {
            if (v.empty() || v.size() != size_t(1 + 2 * int(v[0]))) return 2;
            const int nq = int(v[0]);
            if (make_rule<T>(nq, v.data() + 1, v.data() + 1 + nq, q)) return 2;
            continue;
        }
        if (v.size() < 2) return 2;
        if (cmd == "em") {
            const int d = int(v[0]), drift = int(v[1]);
            if (drift < 0 || drift >= NUM_DRIFTS) return 2;
            bool ok = false;
            if (d == 1) ok = em_case<T, 1>(drift, v);
            else if (d == 2) ok = em_case<T, 2>(drift, v);
            else if (d == 3) ok = em_case<T, 3>(drift, v);
            else if (d == 4) ok = em_case<T, 4>(drift, v);
            if (!ok) return 2;
            continue;
        }
        const int drift = int(v[0]);
        if (drift < 0 || drift >= NUM_DRIFTS || q.nq < 1) return 2;
        Par<T> p{T(v[1])};
        if (cmd == "lin") {
            if (v.size() != 6) return 2;
            T a, b, c;
            if (drift == 0) linearize_point<T, 0>(q, p, T(v[2]), T(v[3]), T(v[4]), T(v[5]), a, b, c);
            else linearize_point<T, 1>(q, p, T(v[2]), T(v[3]), T(v[4]), T(v[5]), a, b, c);
            print(std::vector<T>{a, b, c});
        } else if (cmd == "dd") {
            if (v.size() != 7) return 2;
            T val, gm, gs, ga, gb;
            if (drift == 0) gh_drift_difference<T, 0>(q, p, T(v[2]), T(v[3]), T(v[4]), T(v[5]), T(v[6]), val, gm, gs, ga, gb);
            else gh_drift_difference<T, 1>(q, p, T(v[2]), T(v[3]), T(v[4]), T(v[5]), T(v[6]), val, gm, gs, ga, gb);
            print(std::vector<T>{val, gm, gs, ga, gb});
        } else {
            return 2;
        }
    }
    return 0;
}
}   // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (!std::strcmp(argv[1], "f64")) return run<double>();
    if (!std::strcmp(argv[1], "f32")) return run<float>();
    return 2;
}
