// CPU walk of the moved head carry of the streamed A (markovflow_amd/csrc/mf_head_carry.hpp): Stream<288, KeepAll, true, 4>, its
// decisions (HeadCarry with four tail units) and the two-word per-lane schedule the kernel uses (MovedSchedule), for a whole
// wavefront: 64 rows (one chunk each), every DMA instruction, every lane, step after step.  The LDS image is modelled slot by slot:
// a slot that a masked-out lane leaves alone KEEPS what it held, and at the top of a step - after the consumer has read its row -
// the lane copies the tail units that its NEXT row carries from the tail slots to the head slots.
// Test infrastructure: tests/test_a_head_move_host_sim.py.
#include "../../markovflow_amd/csrc/mf_head_carry.hpp"

#include <cstdint>
#include <set>
#include <vector>

namespace {
using namespace mf;

constexpr int ROWB = 288;
using St = Stream<ROWB, KeepAll, true, 4>;
using HC = St::HC;
using MS = MovedSchedule<St>;
static_assert(St::NT == 4 && St::UB == 18 && St::U == 22 && HC::PERIOD == 4 && MS::USABLE, "the layout the kernel is built for");

// the global byte address a slot holds, the fetch that brought it into LDS, and whether it reached this slot by the in-LDS move
struct Slot { uint64_t src = ~0ull; long fetch = -1; bool moved = false; };

// 64 lanes, lane r owning the chunk of `len` rows that starts at base + r len ROWB.  out[0] = (row, step) pairs walked,
// out[1] = 128-B lines touched by all fetches, out[2] = the same for the plain fetch (own units only, every step),
// out[3] = carried units, out[4] = chunks, out[5] = rows that carried right after a row that carried.  Returns the violations:
//   1  the consumer's schedule differs from the address rule carried_units(row address);
//   2  a unit the consumer reads does not hold the bytes of its row (wrong source address: stale, shifted, lost or never fetched);
//   4  ... or did not come the way the consumer expects: a carried unit by the previous step's fetch and the move, any other
//      unit by this step's fetch into its own slot;
//   8  the fetch of a row touched the line that holds its carried head;
//  16  a unit was fetched although nothing reads it (a carried head unit, or a tail without a consumer) after a chunk's first fetch;
//  32  the move read a tail slot that does not hold the next row's head unit as the fetch of THIS step's rows left it (in
//      particular: a tail slot that a later fetch has already overwritten).
int walk(uint64_t base, long len, double* out) {
    constexpr int P = HC::PERIOD;
    int bad = 0;
    uint64_t addr0[64];
    for (int r = 0; r < 64; ++r) addr0[r] = base + (uint64_t)r * (uint64_t)len * ROWB;
    // the DMA lanes' schedules, built by the function the kernel's DmaStreamMoved::init calls; the consumers'.  The lane-to-unit
    // arithmetic of the FETCH, (row, unit) = divmod(64 i + lane, U), is RESTATED below, not shared with the kernel (mf_kf_lds.hpp
    // does not compile for the host): a change of that mapping in init is caught by tests/test_gpu_kalman_a_head_move.py.
    unsigned w0[64], w1[64];
    for (int l = 0; l < 64; ++l) {
        MS::build(w0[l], w1[l], l, [&](int row) { return (unsigned)addr0[row]; });
        w1[l] = MS::with_consumer(w1[l], (unsigned)addr0[l]);
    }
    std::vector<Slot> image(64 * St::U);
    long lines = 0, lines_plain = 0, carried_n = 0, running = 0;
    for (long j = 0; j < len; ++j) {
        // fetch j: the rows of step j (issued during step j - 1 after that step's move, landed at the top of step j)
        std::set<uint64_t> touched[64];
        bool fetched[64][St::U] = {};
        for (int l = 0; l < 64; ++l) {
            const unsigned mask = MS::fetch_mask(w0[l], w1[l], (unsigned)(j % P));
            for (int i = 0; i < St::NI; ++i) {
                if (j > 0 && !MS::fetch(mask, i)) continue;                            // masked out: the slot keeps its data
                const int p = 64 * i + l, row = p / St::U, cu = p % St::U;
                const uint64_t ua = addr0[row] + (uint64_t)j * ROWB + (uint64_t)St::global_offset(cu);
                image[p] = Slot{ua, j, false};
                fetched[row][cu] = true;
                touched[row].insert(ua >> 7);
                touched[row].insert((ua + St::UNIT - 1) >> 7);
            }
        }
        for (int r = 0; r < 64; ++r) {
            // the consumer reads its row of step j: EVERY unit from the row's own slot
            const uint64_t addr = addr0[r] + (uint64_t)j * ROWB;
            const unsigned rule = j >= 1 ? HC::carried_units((int)(addr & 127)) : 0u;
            const unsigned rule_prev = j >= 2 ? HC::carried_units((int)((addr - ROWB) & 127)) : 0u;
            if (rule != 0u && rule_prev != 0u) ++running;
            std::set<uint64_t> plain;
            for (int u = 0; u < St::UB; ++u) {
                const uint64_t ua = addr + (uint64_t)u * St::UNIT;
                plain.insert(ua >> 7);
                plain.insert((ua + St::UNIT - 1) >> 7);
                const int t = HC::tail_index(u);
                const bool want = t >= 0 && t < St::NT && ((rule >> t) & 1u) != 0u;
                const Slot& s = image[r * St::U + u];
                if (s.src != ua) bad |= 2;
                if (s.fetch != (want ? j - 1 : j) || s.moved != want) bad |= 4;
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
            // the move: the tail units that row j + 1 carries go from the tail slots to the (now dead) head slots
            const unsigned rule_next = HC::carried_units((int)((addr + ROWB) & 127));
            for (int t = 0; t < St::NT; ++t) {
                const bool mv = MS::carried(w1[r], t, (unsigned)((j + 1) % P));
                if (mv != (((rule_next >> t) & 1u) != 0u)) bad |= 1;
                if (!mv) continue;
                const Slot& tail = image[r * St::U + St::UB + t];
                if (tail.src != addr + ROWB + (uint64_t)HC::tail_unit(t) * St::UNIT || tail.fetch != j || tail.moved) bad |= 32;
                image[r * St::U + HC::tail_unit(t)] = Slot{tail.src, tail.fetch, true};
            }
        }
    }
    out[0] = 64.0 * (double)len; out[1] = (double)lines; out[2] = (double)lines_plain; out[3] = (double)carried_n; out[4] = 64.0;
    out[5] = (double)running;
    return bad;
}
}  // namespace

extern "C" {
// {tail slots, period, units per image row, instructions per block, blocks, special units a lane meets per block, fetch bits in
//  word 0, bits used in word 1}
void mf_a_head_move_layout(int* out) {
    out[0] = St::NT; out[1] = HC::PERIOD; out[2] = St::U; out[3] = MS::PER; out[4] = MS::NB; out[5] = MS::NS;
    out[6] = MS::PB * MS::NB * MS::NS; out[7] = MS::SH_C + St::NT * MS::PB;
}
// carried_units(r) for a row that starts r bytes into a line
unsigned mf_a_head_move_rule(int r) { return HC::carried_units(r); }
int mf_a_head_move_walk(uint64_t base, long len, double* out) { return walk(base, len, out); }
}
