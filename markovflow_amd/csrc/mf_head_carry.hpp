// Head carry of a streamed row-major tensor whose rows do not start on 128-B lines (mf_kf_lds.hpp: chol Q, and A where its part of the line is at most 64 B).
//
// A row of ROWB bytes is fetched as the UNIT-byte units that Keep flags.  When a row starts inside a line, that line was already
// touched by the fetch of the previous row (whose last unit ends where this row starts).  If ALL kept units of the row that lie in
// this first line belong to a small fixed set - the "tail units", at most MAXT of them - the previous row's fetch brings them
// along (as extra units past its own end, out of a line it moves anyway), the consumer takes them from there - chol Q: copied to
// registers and held across the step boundary; A: moved inside LDS from the tail slots to the row's own head slots, which the
// row's fetch masks out (MovedSchedule below) - and the row's own fetch leaves the first line alone: one line less on the fabric for that row.
//
// Everything here is integer arithmetic on BYTE ADDRESSES modulo 128 (base offsets, batch slices and chunk starts all shift the
// phase, differently for every lane), shared by the two sides that have to agree:
//   * the consumer: lane r, reading row r of the LDS image at the top of a step, decides per tail unit "carried or in the image";
//   * the producer: the DMA lane that fetches a unit of some OTHER row decides "fetch or leave out" for head and tail units.
// Both derive their decision from carried(address of the row whose head is in question, t): they agree by construction.
// Plain constexpr functions: used by the kernel and, compiled for the host, by tests/host_sim/*head_*_sim.cpp.
#pragma once

namespace mf {

template <int ROWB, int UNIT, typename Keep, int MAXT_ = 2> struct HeadCarry {
    static constexpr int LINE = 128;
    static constexpr int MAXT = MAXT_;                              // tail units per row (each costs 64 x UNIT bytes of LDS)
    static_assert(MAXT >= 1 && MAXT <= 4, "one bit table per tail unit: TAB0 ... TAB3");
    static constexpr int UG = (ROWB + UNIT - 1) / UNIT;             // units per row in global memory
    static constexpr int STEP = ROWB % LINE;                        // the phase advances by this much from one row to the next
    // the t-th candidate: kept units, in order, that can lie wholly inside a first line shared with the previous row
    static constexpr int cand(int t) {
        int n = 0;
        for (int u = 0; u < UG; ++u)
            if (Keep::keep(u, UNIT) && (u + 1) * UNIT <= LINE - 4) { if (n == t) return u; ++n; }
        return -1;
    }
    static constexpr int count_cand() { int n = 0; while (n < MAXT && cand(n) >= 0) ++n; return n; }
    static constexpr int tail_index(int u) { for (int t = 0; t < count_cand(); ++t) if (cand(t) == u) return t; return -1; }
    // Tail units (bit t = unit cand(t)) that a row at byte address r (mod 128) takes from the previous row's fetch.  Empty unless
    // every kept unit that touches the row's first line is a tail unit and lies wholly inside that line: otherwise the row's own
    // fetch moves the line anyway and carrying buys nothing.
    static constexpr unsigned carried_units(int r) {
        r &= LINE - 1;
        if (r == 0) return 0u;                                      // the row starts a line of its own
        const int room = LINE - r;                                  // bytes of the row inside its first line
        unsigned m = 0u;
        for (int u = 0; u < UG; ++u) {
            if (!Keep::keep(u, UNIT) || u * UNIT >= room) continue;
            const int t = tail_index(u);
            if (t < 0 || (u + 1) * UNIT > room) return 0u;
            m |= 1u << t;
        }
        return m;
    }
    // the same as a 32-entry bit table over (r / 4) per tail unit
    static constexpr unsigned table(int t) {
        unsigned m = 0u;
        for (int g = 0; g < 32; ++g) if ((carried_units(4 * g) >> t) & 1u) m |= 1u << g;
        return m;
    }
    static constexpr unsigned TAB0 = table(0), TAB1 = table(1), TAB2 = table(2), TAB3 = table(3);
    // the decisions repeat with this period in the step index (a power of two, at most 32 for rows of whole dwords)
    static constexpr int period() { int p = 1, r = STEP; while (r % LINE) { r += STEP; ++p; } return p; }
    static constexpr int PERIOD = (ROWB % 4 == 0) ? period() : 0;
    // Usable: rows of whole dwords that span at least a line (the line before a row then belongs to the previous row alone) but
    // not a whole number of lines (such rows share no line unless the base is misaligned), whose last unit is fetched (so the
    // previous row's fetch does touch the shared line), and some phase that carries at all.
    static constexpr bool USABLE = ROWB % 4 == 0 && ROWB >= LINE && STEP != 0 && Keep::keep(UG - 1, UNIT) && (TAB0 | TAB1 | TAB2 | TAB3) != 0u;
    static constexpr int NT = USABLE ? count_cand() : 0;
    static constexpr int tail_unit(int t) { return cand(t); }

    // THE decision: is tail unit t of the row at byte address `addr` (its low 7 bits matter) carried from the previous row's fetch?
    static constexpr bool carried(unsigned addr, int t) {
        return (((t == 0 ? TAB0 : t == 1 ? TAB1 : t == 2 ? TAB2 : TAB3) >> ((addr & (LINE - 1)) >> 2)) & 1u) != 0u;
    }

    // Consumer schedule of a lane whose row of step 0 is at addr0: bit (t PERIOD + j % PERIOD) = tail unit t of step j's row is
    // carried (j >= 1; step 0 of a chunk is fetched whole).
    static constexpr unsigned consumer_bits(unsigned addr0) {
        unsigned m = 0u;
        for (int t = 0; t < NT; ++t)
            for (int p = 0; p < PERIOD; ++p) if (carried(addr0 + (unsigned)(p * STEP), t)) m |= 1u << (t * PERIOD + p);
        return m;
    }
    // Producer schedule of a DMA lane that moves one unit of the row whose step-0 address is addr0: bit (jn % PERIOD) = fetch the
    // unit when the rows of step jn >= 1 are fetched.  kind 0: an ordinary unit; 1 + t: the row's own (head) unit tail_unit(t);
    // 1 + MAXT + t: the NEXT row's unit tail_unit(t), fetched into this row's tail slot t.
    static constexpr unsigned producer_bits(unsigned addr0, int kind) {
        unsigned m = 0u;
        for (int p = 0; p < PERIOD; ++p) {
            bool f = true;
            if (kind >= 1 + MAXT) f = carried(addr0 + (unsigned)((p + 1) * STEP), kind - 1 - MAXT);
            else if (kind >= 1) f = !carried(addr0 + (unsigned)(p * STEP), kind - 1);
            if (f) m |= 1u << p;
        }
        return m;
    }
};

// One streamed array: ROWB bytes per (row, step), of which only the units flagged by Keep are fetched.
// UNIT is the DMA granule (16 when ROWB is a multiple of 16, else 4).  The LDS image of a stream is
// row-major [64 rows][U units], filled by U wave-instructions: instruction i, lane l carries unit
// p = 64 i + l, i.e. (row, unit) = divmod(p, U) - consecutive lanes read consecutive 16-B pieces of a row.
// (Rows are NOT padded to an odd stride: the per-lane row reads then take a 2..4-way LDS bank conflict, but
// the kernel reads ~600 B per lane per step, nowhere near LDS bandwidth, while padding would push the
// fp64 d=6 image over a quarter of the CU's 160 KB and cost a wave of occupancy.)
// TAIL: the row's image ends with tail slots that hold the NEXT row's head units (chol Q; A where KfLdsCfg::ATAIL holds).
template <int ROWB, typename Keep, bool TAIL = false, int MAXT = 2> struct Stream {
    // 16-B granules whenever a row holds at least one; a row that is not a whole number of them (odd d) is fetched up
    // to the next 16-B boundary: the extra 4..12 bytes belong to the next row (or lie past the end of the tensor, where
    // the buffer range check returns zeros) and are never read.  Rows then start 4- or 8-byte aligned, which the DMA
    // (dword-aligned dwordx4) accepts.
    static constexpr int UNIT = (ROWB >= 16) ? 16 : 4;
    static constexpr int UG = (ROWB + UNIT - 1) / UNIT;          // units per row in global memory
    static constexpr int count_kept() { int n = 0; for (int u = 0; u < UG; ++u) n += Keep::keep(u, UNIT) ? 1 : 0; return n; }
    using HC = HeadCarry<ROWB, UNIT, Keep, MAXT>;
    static constexpr int UB = count_kept();                       // the row's own units kept in LDS
    static constexpr int NT = TAIL ? HC::NT : 0;                  // tail slots: the next row's units HC::tail_unit(t)
    static constexpr int U = UB + NT;                             // units per row of the LDS image
    static constexpr int NI = U;                                  // DMA wave-instructions per step
    static constexpr int LDS_BYTES = 64 * U * UNIT;
    static constexpr bool ALL = (UB == UG) && NT == 0;
    // global unit index of the c-th kept unit
    static constexpr int global_unit(int c) {
        int n = 0;
        for (int u = 0; u < UG; ++u) if (Keep::keep(u, UNIT)) { if (n == c) return u; ++n; }
        return -1;
    }
    // global byte offset (from the row's start) of the c-th unit of the image: a tail slot reads past the row's end
    static constexpr int global_offset(int c) { return c < UB ? global_unit(c) * UNIT : ROWB + HC::tail_unit(c - UB) * UNIT; }
    // producer kind (HC::producer_bits) of the c-th unit of the image
    static constexpr int unit_kind(int c) {
        if (c >= UB) return 1 + HC::MAXT + (c - UB);
        for (int t = 0; t < NT; ++t) if (global_unit(c) == HC::tail_unit(t)) return 1 + t;
        return 0;
    }
    // compact index of global unit u (must be kept)
    static constexpr int compact_unit(int gu) {
        int n = 0;
        for (int u = 0; u < gu; ++u) n += Keep::keep(u, UNIT) ? 1 : 0;
        return n;
    }
};

// Packed per-lane schedule of a stream with tail slots whose left-out units are left out by the EXEC mask of their DMA instruction
// and whose consumer reads a carried unit from the tail slot itself (A with two tail units, until MovedSchedule below replaced it
// in the kernel; tests/host_sim/a_head_carry_sim.cpp still walks it): a masked-out slot keeps what the previous fetch put there, so a tail slot filled with the rows of step j is
// still intact after the fetch of step j + 1 (a row carries at most every second step) and the consumer reads it from LDS at the
// top of step j + 1.  DMA instruction i, lane l moves image unit (64 i + l) % U: with G = gcd(64, U) a lane meets the units of ONE
// residue mod G, each once in every PER = U / G consecutive instructions ("block"), and at most one unit per residue is a head or
// a tail unit.  So one word describes the lane: bits 0..3 = index in its block of the instruction that holds that unit (15: none),
// bits SH_F + b PB + p = fetch it with the rows of step jn, jn % PB == p, in block b (HeadCarry::producer_bits of the row it
// belongs to), bits SH_C + t PB + p = HeadCarry::consumer_bits of the lane's OWN row.
template <typename St> struct MaskedSchedule {
    using HC = typename St::HC;
    static constexpr int PB = HC::PERIOD > 0 ? HC::PERIOD : 1;
    static constexpr int gcd(int a, int b) { return b == 0 ? a : gcd(b, a % b); }
    static constexpr int G = gcd(64, St::U), PER = St::U / G, NB = (St::NI + PER - 1) / PER;
    static constexpr int SH_F = 4, SH_C = SH_F + NB * PB;
    static constexpr bool one_special_per_residue() {
        for (int c = 0; c < G; ++c) {
            int n = 0;
            for (int u = c; u < St::U; u += G) n += St::unit_kind(u) != 0 ? 1 : 0;
            if (n > 1) return false;
        }
        return true;
    }
    // the source offset of image unit c is c units from the row's start (every unit kept, the tail units are the row's first)
    static constexpr bool linear() { for (int c = 0; c < St::U; ++c) if (St::global_offset(c) != c * St::UNIT) return false; return true; }
    static constexpr bool no_back_to_back_carry() {
        for (int r = 0; r < HC::LINE; r += 4) if (HC::carried_units(r) != 0u && HC::carried_units(r + HC::STEP) != 0u) return false;
        return true;
    }
    static constexpr bool USABLE = St::NT > 0 && PER < 15 && SH_C + St::NT * PB <= 32 && one_special_per_residue() && linear() &&
                                   no_back_to_back_carry();
    static constexpr unsigned none() { return 0xFu | (((1u << (NB * PB)) - 1u) << SH_F); }     // every unit, every phase
    // account for instruction i, in which the lane moves image unit cu of the row whose step-0 byte address is row_addr
    static constexpr unsigned add(unsigned sch, int i, int cu, unsigned row_addr) {
        int kind = 0;
        for (int cc = 0; cc < St::U; ++cc) if (cu == cc && St::unit_kind(cc) != 0) kind = St::unit_kind(cc);
        if (kind == 0) return sch;
        const int sh = SH_F + (i / PER) * PB;
        return (sch & ~(0xFu | (((1u << PB) - 1u) << sh))) | (unsigned)(i % PER) | (HC::producer_bits(row_addr, kind) << sh);
    }
    // is the lane's unit of instruction i fetched with the rows of a step of phase p (= jn % PB, jn >= 1)?
    static constexpr bool fetch(unsigned sch, int i, unsigned p) {
        return (sch & 0xFu) != (unsigned)(i % PER) || ((sch >> (SH_F + (i / PER) * PB + (int)p)) & 1u) != 0u;
    }
    static constexpr unsigned with_consumer(unsigned sch, unsigned own_addr) { return sch | (HC::consumer_bits(own_addr) << SH_C); }
    // does the lane read tail unit t of its row of step j >= 1 (phase p = j % PB) from its tail slot?
    static constexpr bool carried(unsigned sch, int t, unsigned p) { return ((sch >> (SH_C + t * PB + (int)p)) & 1u) != 0u; }
};

// Packed per-lane schedule of a stream with tail slots whose carried head is MOVED back into the row's own slots (mf_kf_lds.hpp, A
// with up to four tail units): at the top of step j, once row j is in registers, the lane copies the tail units that row j + 1
// carries from its tail slots to its head slots, inside LDS.  The head slots are dead then, the fetch of row j + 1 leaves them out
// through the EXEC mask, and the same fetch may refill the tail slots with the head of row j + 2: rows may carry on consecutive
// steps with ONE tail set, and the consumer reads every unit of a row from the row's own slots.
// A lane meets the units of one residue mod G = gcd(64, U), each once per block of PER = U / G instructions, advancing by 64 % U
// units per instruction.  Head and tail units together are a cyclic run of the image (..., U - 1, 0, 1, ...), so the NS of them
// that a lane meets in a block sit at NS consecutive block positions (cyclically) starting at a position `idx` that is the same in
// every block (runs_consecutive() checks both).  Two words describe the lane:
//   w0  bit (p NB NS + b NS + k) = fetch the k-th special unit of block b with the rows of step jn, jn % PB == p
//       (HeadCarry::producer_bits of the row the unit belongs to);
//   w1  bits 0..3 = idx, bits SH_C + t PB + p = HeadCarry::consumer_bits of the lane's OWN row.
// (The one-word form of MaskedSchedule holds one special unit per block; here there are NS = 4, i.e. PB NB NS = 32 fetch bits.)
template <typename St> struct MovedSchedule {
    using HC = typename St::HC;
    static constexpr int PB = HC::PERIOD > 0 ? HC::PERIOD : 1;
    static constexpr int gcd(int a, int b) { return b == 0 ? a : gcd(b, a % b); }
    static constexpr int G = gcd(64, St::U), PER = St::U / G, NB = (St::NI + PER - 1) / PER, ADV = 64 % St::U;
    static constexpr int count_special(int c) { int n = 0; for (int u = c; u < St::U; u += G) n += St::unit_kind(u) != 0 ? 1 : 0; return n; }
    static constexpr int NS = count_special(0);
    static constexpr int SH_C = 4;
    // block position, relative to the position of unit (cu % G), at which a lane meets unit cu
    static constexpr int rel(int cu) { int q = 0, u = cu % G; while (u != cu) { u = (u + ADV) % St::U; ++q; } return q; }
    // the special unit of cu's residue that a lane meets first: every other one follows within NS - 1 positions (-1: no such unit)
    static constexpr int first_special(int c) {
        for (int s = c; s < St::U; s += G) {
            if (St::unit_kind(s) == 0) continue;
            bool ok = true;
            for (int x = c; x < St::U; x += G) if (St::unit_kind(x) != 0 && (rel(x) - rel(s) + PER) % PER >= NS) ok = false;
            if (ok) return s;
        }
        return -1;
    }
    static constexpr bool runs_consecutive() {
        for (int c = 0; c < G; ++c) if (count_special(c) != NS || first_special(c) < 0) return false;
        return St::NI % PER == 0;
    }
    static constexpr bool linear() { for (int c = 0; c < St::U; ++c) if (St::global_offset(c) != c * St::UNIT) return false; return true; }
    static constexpr bool USABLE = St::NT > 0 && PER <= 15 && NS >= 1 && NS <= PER && PB * NB * NS <= 32 && SH_C + St::NT * PB <= 32 &&
                                   runs_consecutive() && linear();
    // the PB bits `bits` (bit p = phase p) spread to the positions of special k of block b
    static constexpr unsigned spread(unsigned bits, int b, int k) {
        unsigned m = 0u;
        for (int p = 0; p < PB; ++p) m |= ((bits >> p) & 1u) << (p * NB * NS + b * NS + k);
        return m;
    }
    template <int C> static constexpr int FIRST_SPECIAL = first_special(C);
    // the first special unit of residue c (a run-time value)
    template <int C = 0> static constexpr int first_of(int c) {
        if constexpr (C + 1 < G) return c == C ? FIRST_SPECIAL<C> : first_of<C + 1>(c);
        else return FIRST_SPECIAL<C>;
    }
    // HeadCarry::producer_bits of the K-th special unit that a lane of residue c meets in a block, for a row at step-0 address addr
    template <int K, int C = 0> static constexpr unsigned bits_of(unsigned addr, int c) {
        constexpr int KIND = St::unit_kind((FIRST_SPECIAL<C> + ADV * K) % St::U);
        static_assert(KIND != 0, "a special unit");
        const unsigned mine = HC::producer_bits(addr, KIND);
        if constexpr (C + 1 < G) return c == C ? mine : bits_of<K, C + 1>(addr, c);
        else return mine;
    }
    template <int BK, typename F> static constexpr void build_special(unsigned& w0, int idx, int lane, F row_addr) {
        if constexpr (BK < NB * NS) {
            constexpr int B = BK / NS, K = BK % NS;
            int q = idx + K;
            q -= q >= PER ? PER : 0;
            const int row = (64 * (B * PER + q) + lane) / St::U;                // DMA instruction i, lane l moves unit 64 i + l
            w0 |= spread(bits_of<K>(row_addr(row), lane % G), B, K);
            build_special<BK + 1>(w0, idx, lane, row_addr);
        }
    }
    // The words of DMA lane `lane`, branch-free (the kernel runs this per lane): row_addr(r) = step-0 byte address of image row r.
    template <typename F> static constexpr void build(unsigned& w0, unsigned& w1, int lane, F row_addr) {
        const int c0 = lane % St::U, first = first_of(lane % G);
        int idx = 0;
        for (int q = 0; q < PER; ++q) idx = ((c0 + ADV * q) % St::U == first) ? q : idx;
        w0 = 0u;
        w1 = (unsigned)idx;
        build_special<0>(w0, idx, lane, row_addr);
    }
    // bit i = the lane's unit of instruction i is fetched with the rows of a step of phase p (= jn % PB, jn >= 1)
    static constexpr unsigned fetch_mask(unsigned w0, unsigned w1, unsigned p) {
        const unsigned left = ~(w0 >> (p * (unsigned)(NB * NS))), idx = w1 & 0xFu;
        unsigned out = 0u;
        for (int b = 0; b < NB; ++b) {
            unsigned x = ((left >> (b * NS)) & ((1u << NS) - 1u)) << idx;                       // the run, from block position idx on
            x = (x | (x >> PER)) & ((1u << PER) - 1u);                                          // ... cyclically
            out |= x << (b * PER);
        }
        return ~out;
    }
    static constexpr bool fetch(unsigned mask, int i) { return ((mask >> i) & 1u) != 0u; }
    static constexpr unsigned with_consumer(unsigned w1, unsigned own_addr) { return w1 | (HC::consumer_bits(own_addr) << SH_C); }
    // does the lane move tail unit t of its row of step j >= 1 (phase p = j % PB) from its tail slot to its head slot (at step j - 1)?
    static constexpr bool carried(unsigned w1, int t, unsigned p) { return ((w1 >> (SH_C + t * PB + (int)p)) & 1u) != 0u; }
};

struct KeepAll { static constexpr bool keep(int, int) { return true; } };
// keep the units of a row-major D x D matrix (element size S) that contain an entry of the lower triangle
template <int D, int S> struct KeepLower {
    static constexpr bool keep(int u, int unit) {
        const int lo = u * unit, hi = lo + unit;                 // byte range of the unit
        for (int i = 0; i < D; ++i) {
            const int a = (i * D) * S, b = (i * D + i + 1) * S;   // bytes of row i's lower part
            if (a < hi && lo < b) return true;
        }
        return false;
    }
};

}  // namespace mf
