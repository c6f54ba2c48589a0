// CPU walk of the head carry of the streamed A (markovflow_amd/csrc/mf_head_carry.hpp): Stream<288, KeepAll, true>, its decisions
// (HeadCarry) and the packed per-lane schedule the kernel uses (MaskedSchedule), for a whole wavefront: 64 rows (one chunk each),
// every DMA instruction, every lane, step after step - with the LDS image modelled slot by slot, so that a slot a masked-out lane
// leaves alone KEEPS what an earlier fetch put there.  Test infrastructure: tests/test_a_head_carry_host_sim.py.
#include "../../markovflow_amd/csrc/mf_head_carry.hpp"

#include <cstdint>
#include <set>
#include <vector>

namespace {
using namespace mf;

constexpr int ROWB = 288;
using St = Stream<ROWB, KeepAll, true>;
using HC = St::HC;
using MS = MaskedSchedule<St>;
static_assert(St::NT == 2 && St::U == 20 && HC::PERIOD == 4 && MS::USABLE, "the layout the kernel is built for");

struct Slot { uint64_t src = ~0ull; long fetch = -1; };       // the global byte address a slot holds, and the fetch that wrote it

// 64 lanes, lane r owning the chunk of `len` rows that starts at base + r len ROWB.  out[0] = (row, step) pairs walked,
// out[1] = 128-B lines touched by all fetches, out[2] = the same for the plain fetch (own units only, every step),
// out[3] = carried units, out[4] = chunks.  Returns the violations:
//   1  the consumer's schedule differs from the address rule carried_units(row address);
//   2  a unit the consumer reads does not hold the bytes of its row (wrong source address: stale, shifted or never fetched);
//   4  ... or was not written by the fetch the consumer expects (tail slot: the previous step's, own slot: this step's) - in
//      particular a tail slot that was written again between the fetch that filled it and the read that uses it;
//   8  the fetch of a row touched the line that holds its carried head;
//  16  a unit was fetched although nothing reads it (a carried head unit, or a tail without a consumer) after a chunk's first fetch.
int walk(uint64_t base, long len, double* out) {
    constexpr int P = HC::PERIOD;
    int bad = 0;
    uint64_t addr0[64];
    for (int r = 0; r < 64; ++r) addr0[r] = base + (uint64_t)r * (uint64_t)len * ROWB;
    // the DMA lanes' schedules, built as DmaStreamMasked::init builds them; the consumers'.  The lane-to-unit arithmetic
    // (row, unit) = divmod(64 i + lane, U) is RESTATED here, not shared with the kernel (mf_kf_lds.hpp does not compile for the
    // host): a change of that mapping in init is caught by tests/test_gpu_kalman_a_head_carry.py, not by this walk.
    unsigned sch[64], csch[64];
    for (int l = 0; l < 64; ++l) {
        sch[l] = MS::none();
        for (int i = 0; i < St::NI; ++i) {
            const int p = 64 * i + l, row = p / St::U, cu = p % St::U;
            sch[l] = MS::add(sch[l], i, cu, (unsigned)addr0[row]);
        }
        csch[l] = MS::with_consumer(0u, (unsigned)addr0[l]);
    }
    std::vector<Slot> image(64 * St::U);
    long lines = 0, lines_plain = 0, carried_n = 0;
    for (long j = 0; j < len; ++j) {
        // fetch j: the rows of step j (issued during step j - 1, landed at the top of step j)
        std::set<uint64_t> touched[64];
        bool fetched[64][St::U] = {};
        for (int i = 0; i < St::NI; ++i)
            for (int l = 0; l < 64; ++l) {
                if (j > 0 && !MS::fetch(sch[l], i, (unsigned)(j % P))) continue;       // masked out: the slot keeps its data
                const int p = 64 * i + l, row = p / St::U, cu = p % St::U;
                const uint64_t ua = addr0[row] + (uint64_t)j * ROWB + (uint64_t)St::global_offset(cu);
                image[p] = Slot{ua, j};
                fetched[row][cu] = true;
                touched[row].insert(ua >> 7);
                touched[row].insert((ua + St::UNIT - 1) >> 7);
            }
        // the consumers read their rows of step j
        for (int r = 0; r < 64; ++r) {
            const uint64_t addr = addr0[r] + (uint64_t)j * ROWB;
            const unsigned rule = j >= 1 ? HC::carried_units((int)(addr & 127)) : 0u;
            std::set<uint64_t> plain;
            for (int u = 0; u < St::UB; ++u) {
                const uint64_t ua = addr + (uint64_t)u * St::UNIT;
                plain.insert(ua >> 7);
                plain.insert((ua + St::UNIT - 1) >> 7);
                const int t = HC::tail_index(u);
                const bool want = j >= 1 && t >= 0 && t < St::NT && MS::carried(csch[r], t, (unsigned)(j % P));
                if (t >= 0 && t < St::NT && want != (((rule >> t) & 1u) != 0u)) bad |= 1;
                const Slot& s = image[r * St::U + (want ? St::UB + t : u)];
                if (s.src != ua) bad |= 2;
                if (s.fetch != (want ? j - 1 : j)) bad |= 4;
                if (want && fetched[r][u]) bad |= 16;
                carried_n += want ? 1 : 0;
            }
            if (rule != 0u && touched[r].count(addr >> 7)) bad |= 8;
            if (j >= 1)
                for (int t = 0; t < St::NT; ++t) {
                    const bool next_wants = ((HC::carried_units((int)((addr + ROWB) & 127)) >> t) & 1u) != 0u;
                    if (fetched[r][St::UB + t] != next_wants) bad |= 16;
                }
            lines += (long)touched[r].size();
            lines_plain += (long)plain.size();
        }
    }
    out[0] = 64.0 * (double)len; out[1] = (double)lines; out[2] = (double)lines_plain; out[3] = (double)carried_n; out[4] = 64.0;
    return bad;
}
}  // namespace

extern "C" {
// {tail slots, tail unit 0, tail unit 1, period, units per image row, instructions per block, blocks, bits used}
void mf_a_head_carry_layout(int* out) {
    out[0] = St::NT; out[1] = HC::tail_unit(0); out[2] = HC::tail_unit(1); out[3] = HC::PERIOD; out[4] = St::U;
    out[5] = MS::PER; out[6] = MS::NB; out[7] = MS::SH_C + St::NT * MS::PB;
}
// carried_units(r) for a row that starts r bytes into a line
unsigned mf_a_head_carry_rule(int r) { return HC::carried_units(r); }
int mf_a_head_carry_walk(uint64_t base, long len, double* out) { return walk(base, len, out); }
}
