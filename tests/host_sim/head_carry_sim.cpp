// CPU walk of the head-carry decisions of the streamed chol Q (markovflow_amd/csrc/mf_head_carry.hpp): the kernel's own layout
// (Stream) and decision helpers (HeadCarry), row after row, as the producer (the DMA lane that fetches a unit) and as the consumer
// (the lane that reads the row) would take them.  Test infrastructure: tests/test_head_carry_host_sim.py.
#include "../../markovflow_amd/csrc/mf_head_carry.hpp"

#include <cstdint>
#include <set>

namespace {
using namespace mf;

// One series of `rows` consecutive rows at byte address `base`, cut into chunks of `len` steps.  out[0] = rows walked,
// out[1] = 128-B lines touched by all fetches, out[2] = the same without tail slots and carries (every kept unit, every step),
// out[3] = carried units, out[4] = chunks (a chunk's first fetch takes its tail slots unconditionally: at most one line more than
// the plain fetch of that row).
// Returns the number of violations:
//   1  the consumer's schedule differs from the address rule carried_units(row address);
//   2  producer and consumer disagree (a carried head unit is fetched as well, or a tail is fetched after the first step of a
//      chunk without a consumer, or is not fetched although the consumer expects it);
//   4  a kept unit of a row is neither fetched into its slot nor carried (or both).
template <int D, int S, bool TAIL> int walk(uint64_t base, long rows, long len, double* out) {
    using St = Stream<D * D * S, KeepLower<D, S>, TAIL>;
    using HC = typename St::HC;
    constexpr int ROWB = D * D * S, P = HC::PERIOD > 0 ? HC::PERIOD : 1;
    int bad = 0;
    long lines = 0, lines_plain = 0, carried_n = 0, chunks = 0;
    for (long k0 = 0; k0 < rows; k0 += len) {
        const uint64_t addr0 = base + (uint64_t)k0 * ROWB;              // the chunk's row of step 0
        const unsigned cbits = St::NT > 0 ? HC::consumer_bits((unsigned)addr0) : 0u;
        bool tail_fetched[HC::MAXT] = {false, false};                   // by the previous step's fetch
        ++chunks;
        for (long j = 0; j < len && k0 + j < rows; ++j) {
            const uint64_t addr = addr0 + (uint64_t)j * ROWB;
            std::set<uint64_t> touched, plain;
            bool now_tail[HC::MAXT] = {false, false};
            bool in_slot[St::U] = {};
            for (int c = 0; c < St::U; ++c) {                           // producer: every unit of this row's image
                const int kind = St::unit_kind(c);
                const bool fetch = j == 0 || St::NT == 0 || ((HC::producer_bits((unsigned)addr0, kind) >> (j % P)) & 1u);
                const uint64_t ua = addr + (uint64_t)St::global_offset(c);
                if (c < St::UB) { plain.insert(ua >> 7); plain.insert((ua + St::UNIT - 1) >> 7); }
                in_slot[c] = fetch;
                if (!fetch) continue;
                touched.insert(ua >> 7);
                touched.insert((ua + St::UNIT - 1) >> 7);
                if (c >= St::UB) now_tail[c - St::UB] = true;
            }
            for (int t = 0; t < St::NT; ++t) {                          // consumer
                const bool want = j >= 1 && ((cbits >> (t * P + (int)(j % P))) & 1u);
                const bool rule = j >= 1 && ((HC::carried_units((int)(addr & 127)) >> t) & 1u);
                if (want != rule) bad |= 1;
                const int c = St::compact_unit(HC::tail_unit(t));
                if (want && in_slot[c]) bad |= 2;                       // fetched AND carried
                if (want && !tail_fetched[t]) bad |= 2;                 // expected, never fetched
                if (!want && tail_fetched[t] && j >= 2) bad |= 2;           // (j == 1: the first fetch took it unasked)
                if (want == in_slot[c]) bad |= 4;                       // exactly one source per kept unit
                carried_n += want ? 1 : 0;
            }
            for (int c = 0; c < St::UB; ++c) if (St::unit_kind(c) == 0 && !in_slot[c]) bad |= 4;
            for (int t = 0; t < HC::MAXT; ++t) tail_fetched[t] = now_tail[t];
            lines += (long)touched.size();
            lines_plain += (long)plain.size();
        }
    }
    out[0] = (double)rows; out[1] = (double)lines; out[2] = (double)lines_plain; out[3] = (double)carried_n; out[4] = (double)chunks;
    return bad;
}
}  // namespace

extern "C" {
// layout facts of Stream<D D S, KeepLower<D, S>, true>: out = {tail slots, tail unit 0, tail unit 1, period, units per image row}
int mf_head_carry_layout(int d, int s, int* out) {
#define MF_CASE(DD, SS) if (d == DD && s == SS) { using St = mf::Stream<DD * DD * SS, mf::KeepLower<DD, SS>, true>; \
        out[0] = St::NT; out[1] = St::HC::tail_unit(0); out[2] = St::HC::tail_unit(1); out[3] = St::HC::PERIOD; out[4] = St::U; return 0; }
    MF_CASE(6, 8) MF_CASE(6, 4) MF_CASE(5, 8) MF_CASE(4, 8) MF_CASE(7, 8) MF_CASE(3, 8)
#undef MF_CASE
    return -1;
}
int mf_head_carry_walk(int d, int s, int tail, uint64_t base, long rows, long len, double* out) {
#define MF_CASE(DD, SS) if (d == DD && s == SS) return tail ? walk<DD, SS, true>(base, rows, len, out) : walk<DD, SS, false>(base, rows, len, out);
    MF_CASE(6, 8) MF_CASE(6, 4) MF_CASE(5, 8) MF_CASE(4, 8) MF_CASE(7, 8) MF_CASE(3, 8)
#undef MF_CASE
    return -1;
}
}
