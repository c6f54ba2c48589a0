// K0, LDS-staged: the streaming form of kf_chunk_kernel for gfx950.
//
// Same math as kf_chunk_kernel (one lane = one (series, time-chunk) sub-problem, register-resident
// partitioned elimination), but the HBM side is re-designed around the memory system:
//
//   * every lane's next transition (A_k, cholQ_k, b_k, H_k, y_k) is brought in by LDS-DMA
//     (`buffer_load_dword[x4] ... lds`): no VGPR staging, and the load of step k+1 is in flight
//     during almost all of step k, so one wavefront per SIMD is enough to cover HBM latency
//     (one exception: with KfLdsCfg::YREG / HREG - fp64, d = 6, m = 1 - y_k and H_k come by plain buffer loads
//     into registers, y four steps per group, H for the step itself, and their room in LDS holds tail slots of A);
//   * one DMA wave-instruction moves 64 x 16 B as contiguous pieces of consecutive rows
//     (lane -> (row, unit) = divmod(64 i + lane, units per row)), i.e. full 128-B lines of the
//     row-major [B, T, d, d] tensors, instead of 64 lanes touching 64 different lines;
//   * the LDS image is row-major with an ODD row stride (in 16-B units) so the per-lane row reads
//     (`ds_read_b128`, lane r reads row r) are bank-conflict free; the pad slot of every row is
//     filled by an out-of-range DMA lane (the buffer range check returns zeros);
//   * only the 16-B units of cholQ_k that hold lower-triangular entries are fetched into LDS.
//
// A workgroup is ONE wavefront (no barriers anywhere); LDS per workgroup is ~39 KB at d=6 fp64, so
// four workgroups (one per SIMD) share a CU's 160 KB.
//
// Chunk convention here: chunk c of a series owns transitions [c L, min((c+1) L, T-1)), transition t
// leads from block t to block t+1; chunk 0 additionally owns block 0 (the prior).  The separator a
// chunk leaves behind is the block its last transition leads to.
#pragma once
#include "mf_kernels.hpp"
#include "mf_head_carry.hpp"
#include <type_traits>
#ifndef MF_PUMPMASK
#define MF_PUMPMASK 63   // bit k: DMA batch k of the next step is issued between arithmetic phases (else up front)
#endif

namespace mf {

typedef int mf_v4i __attribute__((ext_vector_type(4)));

// NOTE the leading `s_nop 4`: hipcc pads no hazards inside an asm string.  When the descriptor (or the LDS
// address) has just been produced by a VALU instruction - v_readfirstlane, or a v_readlane restoring a spilled
// SGPR - a VMEM instruction reading it needs 5 wait states; without them the DMA ran with a stale descriptor
// and silently fetched another stream's rows.
// Cache policy of the wide (A, cholQ) and narrow (b, H, y) streams: experiment knobs, "" = default policy.
#define MF_POLICY_STR_0 ""
#define MF_POLICY_STR_1 " nt"
#define MF_POLICY_STR_2 " sc1"
#define MF_POLICY_STR_3 " sc0 sc1"
#define MF_POLICY_STR_4 " sc0"
#define MF_POLICY_CAT(n) MF_POLICY_STR_##n
#define MF_POLICY_OF(n) MF_POLICY_CAT(n)
#ifndef MF_POLW
#define MF_POLW 1   // A, cholQ: nt - streamed past the L2 so that it keeps the partially used b, H, y lines (measured -6 %)
#endif
#ifndef MF_POLN
#define MF_POLN 0
#endif
#define MF_POLICY_WIDE MF_POLICY_OF(MF_POLW)
#define MF_POLICY_NARROW MF_POLICY_OF(MF_POLN)
// Up to four consecutive DMA instructions of one stream in ONE asm statement (round 4): the leading `s_nop 4`, the save /
// restore of m0 are paid once per group instead of once per instruction (6 -> 3.5 instructions per DMA, 56 DMAs per step at
// d = 6 fp64), and m0 walks from one 1-KB (dwordx4) or 256-B (dword) slice of the LDS image to the next by `s_add_u32` (SCC is
// declared clobbered; one wait state between a write of m0 and the LDS-DMA that reads it, as before).
#define MF_DMA_HEAD "s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
#define MF_DMA_TAIL "s_mov_b32 m0, %0"
#define MF_DMA_X4(v, pol) "buffer_load_dwordx4 " v ", %1, 0 offen" pol " lds\n\t"
#define MF_DMA_X1(v, pol) "buffer_load_dword " v ", %1, 0 offen" pol " lds\n\t"
#define MF_DMA_STEP4 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
#define MF_DMA_STEP1 "s_add_u32 m0, m0, 0x100\n\ts_nop 0\n\t"
template <bool WIDE, int N> MF_DEV void dma_b128_group(mf_v4i srd, unsigned lds_addr, const unsigned* v) {
    unsigned keep;
    static_assert(N >= 1 && N <= 4, "group size");
#define MF_DMA_B128_BODY(POL)                                                                                                       \
    if constexpr (N == 1)                                                                                                           \
        asm volatile(MF_DMA_HEAD MF_DMA_X4("%3", POL) MF_DMA_TAIL : "=&s"(keep) : "s"(srd), "s"(lds_addr), "v"(v[0]) : "memory", "scc"); \
    else if constexpr (N == 2)                                                                                                      \
        asm volatile(MF_DMA_HEAD MF_DMA_X4("%3", POL) MF_DMA_STEP4 MF_DMA_X4("%4", POL) MF_DMA_TAIL                                 \
                     : "=&s"(keep) : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]) : "memory", "scc");                              \
    else if constexpr (N == 3)                                                                                                      \
        asm volatile(MF_DMA_HEAD MF_DMA_X4("%3", POL) MF_DMA_STEP4 MF_DMA_X4("%4", POL) MF_DMA_STEP4 MF_DMA_X4("%5", POL) MF_DMA_TAIL \
                     : "=&s"(keep) : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]), "v"(v[2]) : "memory", "scc");                   \
    else                                                                                                                            \
        asm volatile(MF_DMA_HEAD MF_DMA_X4("%3", POL) MF_DMA_STEP4 MF_DMA_X4("%4", POL) MF_DMA_STEP4 MF_DMA_X4("%5", POL)           \
                     MF_DMA_STEP4 MF_DMA_X4("%6", POL) MF_DMA_TAIL                                                                  \
                     : "=&s"(keep) : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]) : "memory", "scc");
    if (WIDE) { MF_DMA_B128_BODY(MF_POLICY_WIDE) } else { MF_DMA_B128_BODY(MF_POLICY_NARROW) }
#undef MF_DMA_B128_BODY
}
// The same with an EXEC mask per instruction (em[k], wave-uniform): a lane outside the mask moves nothing and its LDS slot KEEPS
// what it held (the out-of-range offset would put zeros there).  EXEC is saved and restored inside the statement.
#define MF_DMA_HEAD_X "s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b64 %1, exec\n\ts_mov_b32 m0, %3\n\t"
#define MF_DMA_TAIL_X "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
#define MF_DMA_X4_X(v, e) "s_mov_b64 exec, " e "\n\ts_nop 0\n\tbuffer_load_dwordx4 " v ", %2, 0 offen" MF_POLICY_WIDE " lds\n\t"
#define MF_DMA_STEP4_X "s_add_u32 m0, m0, 0x400\n\t"
template <int N> MF_DEV void dma_b128_group_masked(mf_v4i srd, unsigned lds_addr, const unsigned* v, const unsigned long long* em) {
    unsigned keep;
    unsigned long long keepx;
    static_assert(N >= 1 && N <= 4, "group size");
    if constexpr (N == 1)
        asm volatile(MF_DMA_HEAD_X MF_DMA_X4_X("%4", "%5") MF_DMA_TAIL_X
                     : "=&s"(keep), "=&s"(keepx) : "s"(srd), "s"(lds_addr), "v"(v[0]), "s"(em[0]) : "memory", "scc");
    else if constexpr (N == 2)
        asm volatile(MF_DMA_HEAD_X MF_DMA_X4_X("%4", "%6") MF_DMA_STEP4_X MF_DMA_X4_X("%5", "%7") MF_DMA_TAIL_X
                     : "=&s"(keep), "=&s"(keepx) : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]), "s"(em[0]), "s"(em[1]) : "memory", "scc");
    else if constexpr (N == 3)
        asm volatile(MF_DMA_HEAD_X MF_DMA_X4_X("%4", "%7") MF_DMA_STEP4_X MF_DMA_X4_X("%5", "%8") MF_DMA_STEP4_X MF_DMA_X4_X("%6", "%9") MF_DMA_TAIL_X
                     : "=&s"(keep), "=&s"(keepx) : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]), "v"(v[2]), "s"(em[0]), "s"(em[1]), "s"(em[2])
                     : "memory", "scc");
    else
        asm volatile(MF_DMA_HEAD_X MF_DMA_X4_X("%4", "%8") MF_DMA_STEP4_X MF_DMA_X4_X("%5", "%9") MF_DMA_STEP4_X MF_DMA_X4_X("%6", "%10")
                     MF_DMA_STEP4_X MF_DMA_X4_X("%7", "%11") MF_DMA_TAIL_X
                     : "=&s"(keep), "=&s"(keepx)
                     : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "s"(em[0]), "s"(em[1]), "s"(em[2]), "s"(em[3])
                     : "memory", "scc");
}
template <int N> MF_DEV void dma_b32_group(mf_v4i srd, unsigned lds_addr, const unsigned* v) {
    unsigned keep;
    static_assert(N >= 1 && N <= 4, "group size");
    if constexpr (N == 1)
        asm volatile(MF_DMA_HEAD MF_DMA_X1("%3", MF_POLICY_NARROW) MF_DMA_TAIL : "=&s"(keep) : "s"(srd), "s"(lds_addr), "v"(v[0]) : "memory", "scc");
    else if constexpr (N == 2)
        asm volatile(MF_DMA_HEAD MF_DMA_X1("%3", MF_POLICY_NARROW) MF_DMA_STEP1 MF_DMA_X1("%4", MF_POLICY_NARROW) MF_DMA_TAIL
                     : "=&s"(keep) : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]) : "memory", "scc");
    else if constexpr (N == 3)
        asm volatile(MF_DMA_HEAD MF_DMA_X1("%3", MF_POLICY_NARROW) MF_DMA_STEP1 MF_DMA_X1("%4", MF_POLICY_NARROW) MF_DMA_STEP1
                     MF_DMA_X1("%5", MF_POLICY_NARROW) MF_DMA_TAIL
                     : "=&s"(keep) : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]), "v"(v[2]) : "memory", "scc");
    else
        asm volatile(MF_DMA_HEAD MF_DMA_X1("%3", MF_POLICY_NARROW) MF_DMA_STEP1 MF_DMA_X1("%4", MF_POLICY_NARROW) MF_DMA_STEP1
                     MF_DMA_X1("%5", MF_POLICY_NARROW) MF_DMA_STEP1 MF_DMA_X1("%6", MF_POLICY_NARROW) MF_DMA_TAIL
                     : "=&s"(keep) : "s"(srd), "s"(lds_addr), "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]) : "memory", "scc");
}

// (Stream, KeepAll, KeepLower: the layout of a streamed array and of its LDS image, in mf_head_carry.hpp.)

constexpr unsigned MF_DMA_INVALID = 0xF0000000u;   // row offset of an invalid row: lands out of range
constexpr unsigned long long MF_DMA_MAXREC = 0xE0000000ull;

// tail slots and schedule period of a stream type (0 / 1 for the types that know nothing of tails)
template <typename St, typename = void> struct StreamTail { static constexpr int NT = 0, PERIOD = 1; };
template <typename St> struct StreamTail<St, std::enable_if_t<(St::NT > 0)>> { static constexpr int NT = St::NT, PERIOD = St::HC::PERIOD; };

// DMA source addressing of one stream.  The per-row byte offsets (relative to the wave's descriptor
// base) live in a 64-entry LDS table; each lane derives its (row, unit) for instruction i from two
// per-lane constants and compile-time (64 i) / U, (64 i) % U - a few VALU ops, no per-instruction
// registers (a register table per instruction was spilled to scratch, and every scratch reload waits
// `vmcnt(0)`, i.e. for every DMA in flight).
template <typename St> struct DmaStream {
    using TL = StreamTail<St>;
    unsigned vo[St::NI];           // this lane's source byte offset for DMA instruction i (registers / AGPRs)
    // head carry (streams with tail slots): PB bits per instruction, bit (jn % PB) = this lane's unit is fetched with the rows of
    // step jn >= 1 (HeadCarry::producer_bits), packed in instruction order
    static constexpr int PB = TL::PERIOD;
    static constexpr int FW = TL::NT > 0 ? (St::NI * PB + 31) / 32 : 1;
    unsigned fm[FW];
    // rel_tab: LDS byte address of this stream's row-offset table; gtab: LDS byte address of the
    // compact-unit -> global byte offset table (only read when the stream drops units)
    // base_lo: low 32 bits of the address the row offsets are relative to (streams with tail slots only: the phase of a row)
    MF_DEV void init(const char* smem, int lane, int rel_tab, int gtab, unsigned base_lo = 0u) {
        const int q0 = lane / St::U, c0 = lane - q0 * St::U;
        if constexpr (TL::NT > 0) { MF_UNROLL for (int w = 0; w < FW; ++w) fm[w] = 0u; }
        MF_UNROLL for (int i = 0; i < St::NI; ++i) {
            const int a = (64 * i) / St::U, b = (64 * i) % St::U;
            int cu = c0 + b;
            const int carry = cu >= St::U ? 1 : 0;
            cu -= carry * St::U;
            const int row = q0 + a + carry;
            const unsigned rel = *reinterpret_cast<const unsigned*>(smem + rel_tab + row * 4);
            unsigned off;
            if (St::ALL) off = (unsigned)cu * St::UNIT;
            else off = *reinterpret_cast<const unsigned*>(smem + gtab + cu * 4);
            vo[i] = rel + off;
            if constexpr (TL::NT > 0) {
                static_assert(PB < 32 && 32 % PB == 0, "an instruction's schedule bits do not straddle two words");
                int kind = 0;
                MF_UNROLL for (int cc = 0; cc < St::U; ++cc) if (St::unit_kind(cc) != 0 && cu == cc) kind = St::unit_kind(cc);
                unsigned bits = (1u << PB) - 1u;
                MF_UNROLL for (int kk = 1; kk <= 2 * St::HC::MAXT; ++kk)
                    if (kind == kk) bits = St::HC::producer_bits(base_lo + rel, kk);
                fm[(i * PB) / 32] |= bits << ((i * PB) % 32);
            }
#ifdef MF_EXPERIMENT
            // ablation "what would a line ring buy" (MF_KF_DEBUG bit 3): bits 24..28 carry the unit's index in its row, bits
            // 29..30 the 32-byte phase of the row's first step (valid offsets stay below 2^24)
            if (pack_base != 0xffffffffu && rel < MF_DMA_INVALID)
                vo[i] |= ((((pack_base + rel) >> 5) & 3u) << 29) | ((unsigned)(off / St::UNIT) << 24);
#endif
        }
    }
#ifdef MF_EXPERIMENT
    unsigned pack_base = 0xffffffffu;     // low 32 bits of the stream's base address when the ablation is on
    unsigned step_next = 0;               // index (within the chunk) of the step whose rows are being fetched
    bool skip_carried = false;
    // the offset actually issued: a unit that lies in the row's first 128-B line, when that line is shared with the previous
    // row (row start not on a line boundary), is NOT fetched (results are garbage - timing / traffic experiment only)
    MF_DEV unsigned exp_offset(unsigned v) const {
        if (pack_base == 0xffffffffu || v >= MF_DMA_INVALID) return v;
        const unsigned phase = ((v >> 29) + step_next) & 3u, gu = (v >> 24) & 31u, off = v & 0xffffffu;
        const bool carried = skip_carried && phase != 0u && gu < 8u - 2u * phase;
        return carried ? MF_DMA_INVALID : off;
    }
#endif
    // issue DMA instructions [i0, i1) of this stream, up to four per asm statement.  SCHED (streams with tail slots, every fetch
    // but a chunk's first): phase = jn % PB of the step jn being fetched; a unit the schedule leaves out gets the out-of-range
    // offset, i.e. zeros in its own slot, which nothing reads.
    template <int I0, int I1, bool SCHED = false> MF_DEV void issue(mf_v4i srd, unsigned lds_base, unsigned phase = 0u) const {
        constexpr int HI = I1 < St::NI ? I1 : St::NI;
        if constexpr (I0 < HI) {
            constexpr int N = (HI - I0) < 4 ? (HI - I0) : 4;
            unsigned voff[N];
            MF_UNROLL for (int k = 0; k < N; ++k) {
#ifdef MF_EXPERIMENT
                voff[k] = exp_offset(vo[I0 + k]);
#else
                voff[k] = vo[I0 + k];
#endif
                if constexpr (SCHED && TL::NT > 0)
                    voff[k] = ((fm[((I0 + k) * PB) / 32] >> (((I0 + k) * PB) % 32 + phase)) & 1u) ? voff[k] : MF_DMA_INVALID;
            }
            if (St::UNIT == 16) dma_b128_group<(St::UG >= 8), N>(srd, lds_base + I0 * 1024, voff);
            else dma_b32_group<N>(srd, lds_base + I0 * 256, voff);
            issue<I0 + N, I1, SCHED>(srd, lds_base, phase);
        }
    }
};

// DmaStream for a stream with tail slots that keeps every unit (A with KfLdsCfg::ATAIL), a type of its own so that DmaStream
// stays what it was for every other stream.  A unit the schedule leaves out is left out by the EXEC mask of its instruction, so
// its slot keeps what it held: a head slot keeps the carried unit that the consumer moved there from the tail slot (see
// MovedSchedule, mf_head_carry.hpp, and the top of MF_KF_LDS_STEP) - no carried values held in registers across the step.  The
// schedule is two packed words per lane, consumer bits included.
template <typename St> struct DmaStreamMoved {
    using MS = MovedSchedule<St>;
    static_assert(MS::USABLE && St::UNIT == 16 && St::UG >= 8, "moved schedule: see MovedSchedule; a wide stream");
    unsigned vo[St::NI];           // this lane's source byte offset for DMA instruction i
    unsigned sch0, sch1;           // the lane's packed schedule
    // base_lo: low 32 bits of the address the row offsets are relative to (the phase of a row); the lane-to-unit arithmetic is
    // DmaStream::init's
    MF_DEV void init(const char* smem, int lane, int rel_tab, int, unsigned base_lo) {
        const int q0 = lane / St::U, c0 = lane - q0 * St::U;
        MS::build(sch0, sch1, lane,
                  [&](int row) { return base_lo + *reinterpret_cast<const unsigned*>(smem + rel_tab + row * 4); });
        MF_UNROLL for (int i = 0; i < St::NI; ++i) {
            const int a = (64 * i) / St::U, b = (64 * i) % St::U;
            int cu = c0 + b;
            const int carry = cu >= St::U ? 1 : 0;
            cu -= carry * St::U;
            const int row = q0 + a + carry;
            const unsigned rel = *reinterpret_cast<const unsigned*>(smem + rel_tab + row * 4);
            const unsigned off = (unsigned)cu * St::UNIT;          // (MovedSchedule::linear)
            vo[i] = rel + off;
#ifdef MF_EXPERIMENT
            if (pack_base != 0xffffffffu && rel < MF_DMA_INVALID)
                vo[i] |= ((((pack_base + rel) >> 5) & 3u) << 29) | ((unsigned)(off / St::UNIT) << 24);
#endif
        }
    }
#ifdef MF_EXPERIMENT
    unsigned pack_base = 0xffffffffu;     // (as in DmaStream)
    unsigned step_next = 0;
    bool skip_carried = false;
    MF_DEV unsigned exp_offset(unsigned v) const {
        if (pack_base == 0xffffffffu || v >= MF_DMA_INVALID) return v;
        const unsigned phase = ((v >> 29) + step_next) & 3u, gu = (v >> 24) & 31u, off = v & 0xffffffu;
        const bool carried = skip_carried && phase != 0u && gu < 8u - 2u * phase;
        return carried ? MF_DMA_INVALID : off;
    }
#endif
    // issue DMA instructions [i0, i1), up to four per asm statement.  SCHED (every fetch but a chunk's first): phase = jn % period
    // of the step jn being fetched; each instruction runs under the ballot of "this lane's unit is fetched".
    template <int I0, int I1, bool SCHED = false> MF_DEV void issue(mf_v4i srd, unsigned lds_base, unsigned phase = 0u) const {
        constexpr int HI = I1 < St::NI ? I1 : St::NI;
        if constexpr (I0 < HI) {
            constexpr int N = (HI - I0) < 4 ? (HI - I0) : 4;
            unsigned voff[N];
            MF_UNROLL for (int k = 0; k < N; ++k) {
#ifdef MF_EXPERIMENT
                voff[k] = exp_offset(vo[I0 + k]);
#else
                voff[k] = vo[I0 + k];
#endif
            }
            if constexpr (SCHED) {
                const unsigned mask = MS::fetch_mask(sch0, sch1, phase);
                unsigned long long em[N];
                MF_UNROLL for (int k = 0; k < N; ++k) em[k] = __builtin_amdgcn_ballot_w64(MS::fetch(mask, I0 + k));
                dma_b128_group_masked<N>(srd, lds_base + I0 * 1024, voff, em);
            } else dma_b128_group<true, N>(srd, lds_base + I0 * 1024, voff);
            issue<I0 + N, I1, SCHED>(srd, lds_base, phase);
        }
    }
};

// value of lane 0 as a wave-uniform (SGPR) 64-bit quantity
MF_DEV unsigned long long uniform64(unsigned long long x) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// wave-uniform buffer descriptor over [base, end)
MF_DEV mf_v4i make_srd(unsigned long long base, unsigned long long end, int debug = 0) {
    unsigned long long rem = end > base ? end - base : 0ull;
    if (debug & 1) rem = 0;
    if (rem > MF_DMA_MAXREC) rem = MF_DMA_MAXREC;
    mf_v4i srd;
    srd.x = __builtin_amdgcn_readfirstlane((int)(unsigned)base);
    srd.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(base >> 32) & 0xffffu));
    srd.z = __builtin_amdgcn_readfirstlane((int)(unsigned)rem);
    srd.w = 0x00020000;
    return srd;
}

// YREG: the next group of this lane's y values, N doubles at byte offset voff of the range-checked descriptor [base, end) - plain
// buffer loads, one dwordx4 per two values (the range check is per dword, as for the DMA: a value past the end reads as zero).
// The compiler counts these loads itself and waits before it first touches their registers - with `vmcnt(n)` of ITS count, which
// knows nothing of the DMA in flight.  So the kernel drains the counter itself at the END of the step that issued them (see
// MF_KF_LDS_STEP): whatever the compiler then adds, for the copies on the loop's back edge, comes after and waits for nothing.
template <typename T, int N> MF_DEV void yreg_load(unsigned long long base, unsigned long long end, int debug, unsigned voff, T (&q)[N]) {
    static_assert(sizeof(T) == 8 && N % 2 == 0, "two values per dwordx4");
    unsigned long long rem = end > base ? end - base : 0ull;
    if (debug & 1) rem = 0;
    if (rem > MF_DMA_MAXREC) rem = MF_DMA_MAXREC;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0,
                                                                        __builtin_amdgcn_readfirstlane((int)(unsigned)rem), 0x00020000);
    MF_UNROLL for (int k = 0; k < N; k += 2) {
        struct Pair { T v[2]; };
        const Pair pr = __builtin_bit_cast(Pair, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(voff + 8u * k), 0, 0));
        q[k] = pr.v[0];
        q[k + 1] = pr.v[1];
    }
}

// the group's values and this lane's byte offset from the wave's descriptor base (nothing where y stays in LDS)
template <typename T, int N, bool ON> struct YRegs { T q[N]; unsigned voff; };
template <typename T, int N> struct YRegs<T, N, false> {};

// read this lane's row from an LDS stream image
template <typename T, typename St> struct RowReader {
    const char* row;
    MF_DEV RowReader(const char* smem, int lds_off, int lane) : row(smem + lds_off + lane * (St::U * St::UNIT)) {}
    // element e of the ORIGINAL row (must lie in a kept unit)
    MF_DEV T at(int e) const {
        const int byte = e * (int)sizeof(T);
        const int gu = byte / St::UNIT;
        const int off = St::compact_unit(gu) * St::UNIT + (byte - gu * St::UNIT);
        return *reinterpret_cast<const T*>(row + off);
    }
    // element k of tail slot t: the next row's unit HC::tail_unit(t)
    MF_DEV T tail_at(int t, int k) const { return *reinterpret_cast<const T*>(row + (St::UB + t) * St::UNIT + k * (int)sizeof(T)); }
};

// RSTEP: the observation precision is a per-step stream [B, T, M, M] (KalmanFilterWithSites / WithSparseSites) instead of
// one shared [M, M] matrix held in registers.
// BG: rows of b and H fetched per DMA batch (the same remedy as YG below, for kernels that have the LDS: the passes of the streamed
// backward, mf_post_lds.hpp MODE 2 and mf_grad_lds.hpp, run two wavefronts per CU and take pairs - a 48-B row touches 1.375 lines,
// a 96-B pair 1.5).
// CARRY (kf_chunk_lds_kernel only): chol Q's image gets tail slots and the kernel carries the shared head of the next row in
// registers (mf_head_carry.hpp) - wherever that set is not empty, the stream already drops units, the schedule bits fit two
// registers and the image still fits FOUR wavefronts per CU (a quarter of 160 KB = 40 960 B).  To make room the offset tables,
// which only DmaStream::init reads (before the first DMA is issued), then lie OVER the image.  Everywhere else, and in the sibling
// kernels that reuse this layout (mf_post_lds.hpp, mf_grad_lds.hpp), the streams and the layout are what they were.
template <typename T, int D, int M, bool RSTEP = false, int BG = 1, bool CARRY = false> struct KfLdsCfg {
    static constexpr int S = sizeof(T);
    static constexpr int BGRP = BG;
    using StA0 = Stream<D * D * S, KeepAll>;
    using StAT = Stream<D * D * S, KeepAll, true, 4>;
    using StC0 = Stream<D * D * S, KeepLower<D, S>>;
    using StCT = Stream<D * D * S, KeepLower<D, S>, true>;
    using Stb = Stream<BG * D * S, KeepAll>;
    using StH = Stream<BG * M * D * S, KeepAll>;
    // y rows are tiny (M S bytes): with one output they are fetched YG steps at a time, so a 128-B line of y is
    // touched every YG-th step instead of every step (the memory side moves whole lines whatever part is used)
    static constexpr int YG = (M == 1) ? 4 : 1;
    using Sty = Stream<YG * M * S, KeepAll>;
    using StR = Stream<M * M * S, KeepAll>;
    static constexpr bool RS = RSTEP;
    static constexpr int QUARTER_CU = (160 * 1024) / 4;
    static constexpr int TABLE_BYTES = 5 * 256 + ((StCT::U * 4 + 15) / 16) * 16;
    static constexpr int IMAGE_T = StA0::LDS_BYTES + StCT::LDS_BYTES + Stb::LDS_BYTES + StH::LDS_BYTES + ((Sty::LDS_BYTES + 15) / 16) * 16 +
                                   (RSTEP ? ((StR::LDS_BYTES + 15) / 16) * 16 : 0);
    static constexpr bool TAIL = CARRY && StCT::NT > 0 && !StC0::ALL && StCT::NI * StCT::HC::PERIOD <= 64 &&
                                 StCT::NT * StCT::HC::PERIOD <= 32 && IMAGE_T <= QUARTER_CU && TABLE_BYTES <= IMAGE_T &&
                                 (StA0::NI + StCT::NI + Stb::NI + StH::NI + Sty::NI + (RSTEP ? StR::NI : 0)) < 64;
    using StC = Stream<D * D * S, KeepLower<D, S>, TAIL>;
    // ATAIL (one output, shared precision, where chol Q carries): y and H leave LDS and the room their images took becomes tail
    // slots of A.  HeadCarry<rows of A, KeepAll> with four tail units carries the whole of a row's part of its first line where
    // that part is at most 64 bytes: units 0 ... 3, 0 ... 2, 0 ... 1, 0 of a row that starts 64, 80, 96, 112 bytes into a line.
    // A's schedule goes through the EXEC mask (DmaStreamMoved) and the consumer moves the carried units from the tail slots to the
    // head slots inside LDS; chol Q's stays as it is.
    // YREG: four values of y per group live in registers, loaded by plain buffer loads.  HREG: the step's own row of H is loaded
    // at the top of the step by plain buffer loads into the registers that hold it anyway; the step drains the counter in front
    // of the row's first use (Obs::apply) instead of at its end.
    static constexpr int Y_IMAGE = ((Sty::LDS_BYTES + 15) / 16) * 16;
    static constexpr bool ATAIL = TAIL && M == 1 && !RSTEP && sizeof(T) == 8 && StAT::NT > 0 && StAT::HC::PERIOD == StCT::HC::PERIOD &&
                                  (M * D * S) % 16 == 0 && StAT::LDS_BYTES + StCT::LDS_BYTES + Stb::LDS_BYTES <= QUARTER_CU &&
                                  (StAT::NI + StCT::NI + Stb::NI + (M * D * S) / 16 + (YG * M * S) / 16) < 64;
    static constexpr bool YREG = ATAIL, HREG = ATAIL;
    // (groups of two - one dwordx4, a y line touched every second step - were measured and lost the whole gain)
    static_assert(YG % 2 == 0 || !YREG, "whole dwordx4 loads");
    using DA = std::conditional_t<ATAIL, DmaStreamMoved<StAT>, DmaStream<StA0>>;
    using StA = std::conditional_t<ATAIL, StAT, StA0>;
    static constexpr int NI_y = YREG ? 0 : Sty::NI;
    static constexpr int NI_H = HREG ? 0 : StH::NI;
    static constexpr int OFF_A = 0;
    static constexpr int OFF_C = OFF_A + StA::LDS_BYTES;
    static constexpr int OFF_b = OFF_C + StC::LDS_BYTES;
    static constexpr int OFF_H = OFF_b + Stb::LDS_BYTES;
    static constexpr int OFF_y = OFF_H + (HREG ? 0 : StH::LDS_BYTES);
    static constexpr int OFF_R = OFF_y + (YREG ? 0 : Y_IMAGE);
    static constexpr int IMAGE_END = OFF_R + (RSTEP ? ((StR::LDS_BYTES + 15) / 16) * 16 : 0);
    static constexpr int OFF_relA = TAIL ? 0 : IMAGE_END;                                       // row offsets of A and cholQ
    static constexpr int OFF_relb = OFF_relA + 256;
    static constexpr int OFF_relH = OFF_relb + 256;
    static constexpr int OFF_rely = OFF_relH + 256;
    static constexpr int OFF_relR = OFF_rely + 256;
    static constexpr int OFF_gtabC = OFF_relR + 256;
    static constexpr int LDS_TOTAL = TAIL ? IMAGE_END : OFF_gtabC + ((StC::U * 4 + 15) / 16) * 16;
    // the streaming kernel is instantiated only where matrix rows are whole 16-B units, the per-step DMA count
    // fits the 6-bit vm counter and the image fits 64 KB of LDS
    static constexpr bool SUPPORTED =
                                      (StA::NI + StC::NI + Stb::NI + NI_H + NI_y + (RSTEP ? StR::NI : 0)) < 64 &&
                                      LDS_TOTAL <= 64 * 1024;
};

template <typename T, int D, int M, bool RSTEP = false> using KfChunkCfg = KfLdsCfg<T, D, M, RSTEP, 1, true>;
static_assert(KfChunkCfg<double, 6, 1>::TAIL && KfChunkCfg<double, 6, 1>::LDS_TOTAL <= 40960, "fp64 d = 6: four wavefronts per CU");
static_assert(KfChunkCfg<double, 6, 1>::ATAIL && KfChunkCfg<double, 6, 1>::StA::U == 22 && KfChunkCfg<double, 6, 1>::LDS_TOTAL == 39936,
              "fp64 d = 6, m = 1: A's four tail slots take the place of the y and H images, one unit per lane to spare");
static_assert(KfChunkCfg<double, 6, 1>::StA::NI + KfChunkCfg<double, 6, 1>::StC::NI + KfChunkCfg<double, 6, 1>::Stb::NI == 39,
              "39 LDS-DMA instructions, 3 loads of H and 2 of y per step: 44 in flight, below the 6-bit counter's 63");
static_assert(!KfChunkCfg<double, 6, 2>::ATAIL && !KfChunkCfg<double, 6, 1, true>::ATAIL && !KfChunkCfg<float, 6, 1>::ATAIL &&
              !KfLdsCfg<double, 6, 1>::ATAIL && !KfLdsCfg<double, 6, 1, false, 2>::ATAIL, "every other instantiation keeps its streams");

// DMA batches of one step.  All of a step's data is pulled into registers at the top of the step behind ONE
// `s_waitcnt vmcnt(0)`; the batches of the next step are then issued between the arithmetic phases.
// (Counted waits - "all but the youngest n have landed" - were tried and are NOT safe here: with dword and
// dwordx4 LDS-DMA mixed in one stream of requests the landing order did not follow the issue order.)
template <typename Cfg> struct KfPump {
    static constexpr int N_SMALL = Cfg::StC::NI + Cfg::Stb::NI + Cfg::NI_H + Cfg::NI_y + (Cfg::RS ? Cfg::StR::NI : 0);
    static constexpr bool HREG = Cfg::HREG;   // kf_lds_step drains the vector-memory counter in front of the first use of H
    static constexpr int N_BIG = Cfg::StA::NI;
    const typename Cfg::DA& dA; const DmaStream<typename Cfg::StC>& dC;
    const DmaStream<typename Cfg::Stb>& db; const DmaStream<typename Cfg::StH>& dH;
    const DmaStream<typename Cfg::Sty>& dy; const DmaStream<typename Cfg::StR>& dR;
    mf_v4i sA, sC, sb, sH, sy, sR;
    unsigned lds0;
    bool more;
    bool yfetch = true;     // this step's batch includes the next group of y rows
    unsigned cphase = 0;    // head carry: (index of the step being fetched) % period
    template <int K> MF_DEV void small() const {
        if (!((MF_PUMPMASK >> K) & 1)) return;
        small_do<K>();
    }
    template <int K> MF_DEV void small_do() const {
        if (!more) return;
        constexpr int HC = (Cfg::StC::NI + 1) / 2;
        if (K == 0) dC.template issue<0, HC, true>(sC, lds0 + Cfg::OFF_C, cphase);
        else {
            dC.template issue<HC, 64, true>(sC, lds0 + Cfg::OFF_C, cphase);
            db.template issue<0, 64>(sb, lds0 + Cfg::OFF_b);
            if constexpr (!Cfg::HREG) dH.template issue<0, 64>(sH, lds0 + Cfg::OFF_H);
            if constexpr (!Cfg::YREG) { if (yfetch) dy.template issue<0, 64>(sy, lds0 + Cfg::OFF_y); }
            if (Cfg::RS) dR.template issue<0, 64>(sR, lds0 + Cfg::OFF_R);
        }
    }
    // a chunk's first fetch: every unit, tail slots included (step 0 consumes no carry)
    template <int K> MF_DEV void all() const {
        dC.template issue<0, 64>(sC, lds0 + Cfg::OFF_C);
        db.template issue<0, 64>(sb, lds0 + Cfg::OFF_b);
        if constexpr (!Cfg::HREG) dH.template issue<0, 64>(sH, lds0 + Cfg::OFF_H);
        if constexpr (!Cfg::YREG) dy.template issue<0, 64>(sy, lds0 + Cfg::OFF_y);
        if (Cfg::RS) dR.template issue<0, 64>(sR, lds0 + Cfg::OFF_R);
        dA.template issue<0, 64>(sA, lds0 + Cfg::OFF_A);
    }
    template <int K> MF_DEV void big() const {
        if (!((MF_PUMPMASK >> (K + 2)) & 1)) return;
        big_do<K>();
    }
    // the batches that are NOT pumped between the arithmetic phases are issued up front
    MF_DEV void unpumped() const {
        if (!((MF_PUMPMASK >> 0) & 1)) small_do<0>();
        if (!((MF_PUMPMASK >> 1) & 1)) small_do<1>();
        if (!((MF_PUMPMASK >> 2) & 1)) big_do<0>();
        if (!((MF_PUMPMASK >> 3) & 1)) big_do<1>();
        if (!((MF_PUMPMASK >> 4) & 1)) big_do<2>();
        if (!((MF_PUMPMASK >> 5) & 1)) big_do<3>();
    }
    template <int K> MF_DEV void big_do() const {
        if (!more) return;
        constexpr int Q = (Cfg::StA::NI + 3) / 4;
        if constexpr (Cfg::ATAIL) dA.template issue<K * Q, (K + 1) * Q, true>(sA, lds0 + Cfg::OFF_A, cphase);
        else dA.template issue<K * Q, (K + 1) * Q>(sA, lds0 + Cfg::OFF_A);
    }
};

// One transition of the chain for this lane.  FIRST_SEP: the block on the left is this chunk's separator
// (it is not eliminated here; its coupling seeds the spike).  Register discipline: the only large live
// temporaries are Ci (lower), and ONE D x D array that is A -> B = C^-1 A -> Y = B L^-T -> W in turn;
// Q_k^-1 + H^T R^-1 H is formed after the elimination, when B is no longer needed.
// `pump` issues the LDS-DMA of the NEXT step in small batches between the arithmetic phases: a burst of
// ~40 wave-instructions back to back fills the CU's address queue and stalls the (only) wave of the SIMD
// at issue, while one batch every few hundred VALU instructions is absorbed for free.
// HREG pumps (KfPump of a KfLdsCfg::HREG configuration): the step's row of H was loaded into hk by plain buffer loads at the top of
// the step.  The step then drains the vector-memory counter itself, in full, right in front of the first use of hk - a compiler
// wait there would carry the compiler's count, which knows nothing of the DMA in flight - and pins the compiler's own wait behind it.
template <typename Pump, typename = void> struct PumpHreg { static constexpr bool value = false; };
template <typename Pump> struct PumpHreg<Pump, std::enable_if_t<Pump::HREG>> { static constexpr bool value = true; };
template <typename T, int N> MF_DEV void hreg_arrive(T (&h)[N], const T (&hk)[N]) {
    // (the asm statements are ordered among themselves only: without the barrier the scheduler draws the drain and the
    // observation update far up into the arithmetic that is meant to cover the last batch of A)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    MF_UNROLL for (int i = 0; i < N; ++i) h[i] = hk[i];
    MF_UNROLL for (int i = 0; i < N; ++i) asm volatile("" : "+v"(h[i]));
}

template <typename T, int D, int M, bool SPIKE, bool FIRST, typename Pump>
MF_DEV void kf_lds_step(Elim<T, D, SPIKE>& E, LogAcc<T>& laC, T& acc_yry, T& acc_ww, const T (&C)[D][D],
                        const T (&mvec)[D], const T (&hk)[M * D], const T (&yk)[M], const T (&Rsh)[M * M],
                        T (&Bm)[D][D], const Pump& pump, bool active, bool sep_lane) {
    // FIRST (step 0 of a chunk): lanes of chunks c > 0 take the separator form, lanes of chunk 0 the ordinary
    // one - both inside the SAME call, because the DMA batches must be issued once, by all lanes, in order.
    const bool sep = FIRST && sep_lane, ord = active && !sep;
    // Every arithmetic phase is predicated on `active` (a chunk shorter than the wave's trip count idles),
    // the DMA batches in between are issued by ALL lanes: an LDS-DMA lane carries another row's data.
    T Ci[D][D], w[D], btw[D];
    if (active) {
        tri_inv_lower<T, D>(C, Ci, laC, E.bad);
        laC.renorm();
    }
    pump.template small<0>();
    if (active) {
        trimul_lower_vec<T, D>(Ci, mvec, w);
        acc_ww += dot_self<T, D>(w);
    }
    pump.template small<1>();
    pump.template big<0>();
    if (active) {
        trimul_lower_inplace<T, D, D>(Ci, Bm);            // B = C^-1 A
        gemv_t<T, D, D>(Bm, w, btw);
    }
    pump.template big<1>();
    if (FIRST && active && sep) {
        syrk_tn_lower<T, D, D>(Bm, E.GU, T(1));
        MF_UNROLL for (int i = 0; i < D; ++i) E.gU[i] = -btw[i];
    }
    if (ord) {
        syrk_tn_lower<T, D, D>(Bm, E.Phi, T(1));
        MF_UNROLL for (int i = 0; i < D; ++i) E.t[i] -= btw[i];
    }
    pump.template big<2>();
    if (FIRST && active && sep) {
        neg_trimulT_lower_inplace<T, D, D>(Ci, Bm);       // S = -C^-T B
        MF_UNROLL for (int i = 0; i < D; ++i) MF_UNROLL for (int j = 0; j < D; ++j) E.X[i][j] = Bm[i][j];
    }
    if (ord) E.eliminate_main();
    pump.template big<3>();
    // HREG: H arrives in h.  A chunk's first step takes it ONCE, in front of its two forms: the compiler then shares the products
    // of H, R and y between them as it does where H comes from LDS - with H arriving inside each form it paired the fused
    // multiply-adds of Obs::apply differently and the results moved in the last bits.  Every later step takes it inside the one
    // form it has, behind the arithmetic that covers the last batch of A.
    constexpr bool HR = PumpHreg<Pump>::value;
    T h[HR ? M * D : 1];
    if constexpr (HR && FIRST) hreg_arrive(h, hk);
    if (FIRST && active && sep) {
        trimulT_self_lower<T, D>(Ci, E.Phi);
        trimulT_lower_vec<T, D>(Ci, w, E.t);
        if constexpr (HR) acc_yry += Obs<T, D, M>::apply(h, yk, Rsh, M, E.Phi, E.t);
        else acc_yry += Obs<T, D, M>::apply(hk, yk, Rsh, M, E.Phi, E.t);
    }
    if (ord) {
        E.eliminate_spike();
        trsm_right_lower_t<T, D, D>(E.Phi, E.Li, Bm);     // Y = B L^-T
        neg_trimulT_lower_inplace<T, D, D>(Ci, Bm);       // W = -C^-T Y
        T Dn[D][D], rn[D];
        trimulT_self_lower<T, D>(Ci, Dn);
        trimulT_lower_vec<T, D>(Ci, w, rn);
        if constexpr (HR) {
            if constexpr (!FIRST) hreg_arrive(h, hk);
            acc_yry += Obs<T, D, M>::apply(h, yk, Rsh, M, Dn, rn);
        } else acc_yry += Obs<T, D, M>::apply(hk, yk, Rsh, M, Dn, rn);
        E.advance(Bm, Dn, rn);
    }
}

// KfArgs::P = chunks per series, L = transitions per chunk.
template <typename T, int D, int M, bool SPIKE, bool RSTEP = false>
__global__ void __launch_bounds__(64) kf_chunk_lds_kernel(KfArgs<T> a, long L, RedSys<T> out) {
    using Cfg = KfChunkCfg<T, D, M, RSTEP>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const long total = a.B * a.P;
    const long id_raw = (long)blockIdx.x * 64 + lane;
    const bool valid = id_raw < total;
    const long id = valid ? id_raw : total - 1;
    const long s = id / a.P, c = id % a.P;
    const long nt = a.Tn - 1;                       // transitions per series
    const long tau0 = c * L;
    long len = nt - tau0;
    if (len > L) len = L;
    if (len < 0 || !valid) len = 0;
    constexpr int S = sizeof(T);

    // ---- DMA set-up: per-row offsets into LDS tables, wave-uniform stream pointers ---------------------
    const unsigned long long offA = (unsigned long long)(s * nt + tau0) * (D * D * S);
    const unsigned long long offb = (unsigned long long)(s * nt + tau0) * (D * S);
    const unsigned long long offH = (unsigned long long)(s * a.Tn + tau0 + 1) * (M * D * S);
    const unsigned long long offy = (unsigned long long)(s * a.Tn + tau0 + 1) * (M * S);
    const unsigned long long offR = (unsigned long long)(s * a.Tn + tau0 + 1) * (M * M * S);
    const unsigned long long offA0 = uniform64(offA), offb0 = uniform64(offb);
    const unsigned long long offH0 = uniform64(offH), offy0 = uniform64(offy), offR0 = uniform64(offR);
    const bool rowok = valid && len > 0;
    {
        unsigned* tab = reinterpret_cast<unsigned*>(smem);
        tab[Cfg::OFF_relA / 4 + lane] = rowok ? (unsigned)(offA - offA0) : MF_DMA_INVALID;
        tab[Cfg::OFF_relb / 4 + lane] = rowok ? (unsigned)(offb - offb0) : MF_DMA_INVALID;
        tab[Cfg::OFF_relH / 4 + lane] = rowok ? (unsigned)(offH - offH0) : MF_DMA_INVALID;
        tab[Cfg::OFF_rely / 4 + lane] = rowok ? (unsigned)(offy - offy0) : MF_DMA_INVALID;
        tab[Cfg::OFF_relR / 4 + lane] = rowok ? (unsigned)(offR - offR0) : MF_DMA_INVALID;
        if (lane < Cfg::StC::U) {
            unsigned g = 0;
            MF_UNROLL for (int cc = 0; cc < Cfg::StC::U; ++cc) if (lane == cc) g = (unsigned)Cfg::StC::global_offset(cc);
            tab[Cfg::OFF_gtabC / 4 + lane] = g;
        }
    }
    typename Cfg::DA dA;
    DmaStream<typename Cfg::StC> dC;
    DmaStream<typename Cfg::Stb> db;
    DmaStream<typename Cfg::StH> dH;
    DmaStream<typename Cfg::Sty> dy;
    DmaStream<typename Cfg::StR> dR;
    unsigned long long pA = (unsigned long long)a.A + offA0, pC = (unsigned long long)a.cholQ + offA0;
    unsigned long long pb = (unsigned long long)a.b + offb0, pH = (unsigned long long)a.H + offH0;
    unsigned long long py = (unsigned long long)a.y + offy0;
    unsigned long long pR = (unsigned long long)a.Rinv + (RSTEP ? offR0 : 0ull);
    const unsigned long long eA = (unsigned long long)a.A + (unsigned long long)a.B * nt * (D * D * S);
    const unsigned long long eC = (unsigned long long)a.cholQ + (unsigned long long)a.B * nt * (D * D * S);
    const unsigned long long eb = (unsigned long long)a.b + (unsigned long long)a.B * nt * (D * S);
    const unsigned long long eH = (unsigned long long)a.H + (unsigned long long)a.B * a.Tn * (M * D * S);
    const unsigned long long ey = (unsigned long long)a.y + (unsigned long long)a.B * a.Tn * (M * S);
    const unsigned long long eR = (unsigned long long)a.Rinv + (RSTEP ? (unsigned long long)a.B * a.Tn * (M * M * S) : 0ull);
    const unsigned lds0 = (unsigned)(size_t)smem;

    // ---- block 0 of chunk 0: the prior (plain loads; no DMA in flight yet) ------------------------------
    Elim<T, D, SPIKE> E;
    E.init();
    LogAcc<T> laC;
    laC.init();
    T acc_yry = T(0), acc_ww = T(0);
    T Rsh[M * M];                                  // observation precision: shared (kept in registers) or this step's
    MF_UNROLL for (int i = 0; i < M * M; ++i) Rsh[i] = RSTEP ? (valid ? a.Rinv[(s * a.Tn) * M * M + i] : T(0)) : a.Rinv[i];
    if (valid && c == 0) {
        T C[D][D], Ci[D][D], mvec[D], w[D];
        load_lower<T, D>(a.cholP0 + s * D * D, C);
        load_vec<T, D>(a.mu0 + s * D, mvec);
        tri_inv_lower<T, D>(C, Ci, laC, E.bad);
        laC.renorm();
        trimul_lower_vec<T, D>(Ci, mvec, w);
        acc_ww += dot_self<T, D>(w);
        trimulT_self_lower<T, D>(Ci, E.Phi);
        trimulT_lower_vec<T, D>(Ci, w, E.t);
        acc_yry += Obs<T, D, M>::apply(a.H + (s * a.Tn) * M * D, a.y + (s * a.Tn) * M, Rsh, M, E.Phi, E.t);
    }

    // wave-uniform trip count: the longest chunk in this wave
    long nsteps = len;
    MF_UNROLL for (int off = 32; off > 0; off >>= 1) {
        const long o = __shfl_xor((long long)nsteps, off);
        nsteps = o > nsteps ? o : nsteps;
    }
    nsteps = __builtin_amdgcn_readfirstlane((int)nsteps);
    // the LDS tables must be visible to every lane before the first DMA address is formed (one wave: a
    // wait on the LDS counter is enough) and the plain loads above must be done before DMAs are counted
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#ifdef MF_EXPERIMENT
    if (a.debug & 8) {
        dA.pack_base = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)pA);
        dC.pack_base = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)pC);
    }
#endif
    if constexpr (Cfg::ATAIL) dA.init(smem, lane, Cfg::OFF_relA, 0, (unsigned)pA);
    else dA.init(smem, lane, Cfg::OFF_relA, 0);
    dC.init(smem, lane, Cfg::OFF_relA, Cfg::OFF_gtabC, (unsigned)pC);
    db.init(smem, lane, Cfg::OFF_relb, 0);
    if constexpr (!Cfg::HREG) dH.init(smem, lane, Cfg::OFF_relH, 0);
    if constexpr (!Cfg::YREG) dy.init(smem, lane, Cfg::OFF_rely, 0);
    if (RSTEP) dR.init(smem, lane, Cfg::OFF_relR, 0);
    // (with the head carry the tables lie over the image: the last table read is done before the first DMA writes there)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // head carry: this lane's consumer schedule, and the carried entries of the next row's chol Q (tail slot t, element k)
    using HC = typename Cfg::StC::HC;
    constexpr int NTAIL = Cfg::StC::NT, CPER = NTAIL > 0 ? HC::PERIOD : 1, UEL = Cfg::StC::UNIT / S;
    const unsigned cbits = NTAIL > 0 ? HC::consumer_bits((unsigned)((unsigned long long)a.cholQ + offA)) : 0u;
    T cv[NTAIL > 0 ? NTAIL : 1][UEL];
    MF_UNROLL for (int t = 0; t < (NTAIL > 0 ? NTAIL : 1); ++t) MF_UNROLL for (int k = 0; k < UEL; ++k) cv[t][k] = T(0);

    // A's head carry: the consumer schedule rides in dA's second schedule word; the lane moves the carried units of its next row
    // from the tail slots to the head slots (MF_KF_LDS_STEP) and reads every row from the row's own slots
    using HCA = typename Cfg::StA::HC;
    constexpr int NTA = Cfg::StA::NT;
    if constexpr (NTA > 0) {
        static_assert(HCA::PERIOD == CPER, "one phase for both schedules");
        dA.sch1 = MovedSchedule<typename Cfg::StA>::with_consumer(dA.sch1, (unsigned)((unsigned long long)a.A + offA));
    }
    // YREG: this lane's group of y values (steps YG g ... YG g + YG - 1 of its chunk) and its offset from the wave's descriptor base
    YRegs<T, Cfg::YG * M, Cfg::YREG> yr;
    if constexpr (Cfg::YREG) {
        MF_UNROLL for (int i = 0; i < Cfg::YG * M; ++i) yr.q[i] = T(0);
        yr.voff = rowok ? (unsigned)(offy - offy0) : MF_DMA_INVALID;
    }
    // HREG: this lane's offset of its row of H from the wave's descriptor base (the descriptor advances by a row per step)
    unsigned hvoff = 0u;
    if constexpr (Cfg::HREG) hvoff = rowok ? (unsigned)(offH - offH0) : MF_DMA_INVALID;

    const RowReader<T, typename Cfg::StA> rA(smem, Cfg::OFF_A, lane);
    const RowReader<T, typename Cfg::StC> rC(smem, Cfg::OFF_C, lane);
    const RowReader<T, typename Cfg::Stb> rb(smem, Cfg::OFF_b, lane);
    const RowReader<T, typename Cfg::StH> rH(smem, Cfg::OFF_H, lane);
    const RowReader<T, typename Cfg::Sty> ry(smem, Cfg::OFF_y, lane);
    const RowReader<T, typename Cfg::StR> rR(smem, Cfg::OFF_R, lane);

    using Pump = KfPump<Cfg>;

    if (nsteps > 0) {   // prologue: fetch step 0
        Pump p0{dA, dC, db, dH, dy, dR, make_srd(pA, eA, a.debug), make_srd(pC, eC, a.debug | ((a.debug >> 2) & 1)),
                make_srd(pb, eb, a.debug | ((a.debug >> 1) & 1)), make_srd(pH, eH, a.debug | ((a.debug >> 1) & 1)),
                make_srd(py, ey, a.debug | ((a.debug >> 1) & 1)), make_srd(pR, eR, a.debug | ((a.debug >> 1) & 1)), lds0, true};
        p0.template all<0>();
        if constexpr (Cfg::YREG) yreg_load(py, ey, a.debug | ((a.debug >> 1) & 1), yr.voff, yr.q);
    }

    // One streamed step: wait for this step's cholQ/b/H/y (A may still be in flight), move them to registers,
    // then run the arithmetic with the next step's DMA pumped in between.  FIRST distinguishes step 0 (whose
    // left block is the separator for every chunk but the first) so that the steady-state loop body holds a
    // single code path.
#ifdef MF_STAMP
#define MF_STAMP_AT(var) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); var = t_; }
    unsigned long long st_wait = 0, st_io = 0, st_comp = 0, ts0 = 0, ts1 = 0, ts2 = 0, ts3 = 0;
#define MF_STAMP_ACC { asm volatile("" :: "v"(E.quad), "v"(E.Phi[0][0]) : "memory"); MF_STAMP_AT(ts3) st_wait += ts1 - ts0; st_io += ts2 - ts1; st_comp += ts3 - ts2; }
#else
#define MF_STAMP_AT(var)
#define MF_STAMP_ACC
#endif
#ifdef MF_CHECKSUM
    T cs_A = 0, cs_C = 0, cs_b = 0, cs_H = 0, cs_y = 0;
#define MF_CHECKSUM_ACC if (j < len) { MF_UNROLL for (int i = 0; i < D; ++i) { cs_b += mvec[i]; MF_UNROLL for (int jj = 0; jj < D; ++jj) { cs_A += Bm[i][jj] * T(1 + i * D + jj); if (jj <= i) cs_C += C[i][jj] * T(1 + i * D + jj); } } \
        MF_UNROLL for (int i = 0; i < M * D; ++i) cs_H += hk[i] * T(1 + i); MF_UNROLL for (int i = 0; i < M; ++i) cs_y += yk[i]; }
#else
#define MF_CHECKSUM_ACC
#endif
#ifdef MF_EXPERIMENT
#define MF_EXP_STEP_NEXT { dA.step_next = dC.step_next = (unsigned)(j + 1); dA.skip_carried = dC.skip_carried = (a.debug & 8) != 0; }
#else
#define MF_EXP_STEP_NEXT
#endif
#define MF_NOPUMP_ISSUE pump.unpumped();
#define MF_KF_LDS_STEP(FIRST)                                                                                         \
    {                                                                                                                 \
        MF_STAMP_AT(ts0)                                                                                              \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                              \
        MF_STAMP_AT(ts1)                                                                                              \
        const bool more = (j + 1 < nsteps);                                                                           \
        const bool yfetch = ((j + 1) % Cfg::YG) == 0;                                                                \
        pA += D * D * S; pC += D * D * S; pb += D * S; pH += M * D * S; if (RSTEP) pR += M * M * S;                   \
        if (yfetch) py += Cfg::YG * M * S;                                                                           \
        T C[D][D], mvec[D], hk[M * D], yk[M];                                                                         \
        MF_UNROLL for (int i = 0; i < D; ++i) MF_UNROLL for (int jj = 0; jj <= i; ++jj) C[i][jj] = rC.at(i * D + jj); \
        if constexpr (NTAIL > 0) {                                                                                    \
            /* entries of the row's head units that the previous step carried come from registers; then pick up  */   \
            /* the next row's from the tail slots (zeros where this step's fetch left them out: not used then)   */   \
            MF_UNROLL for (int t = 0; t < NTAIL; ++t) {                                                               \
                const bool got = !(FIRST) && ((cbits >> (t * CPER + (int)(j & (CPER - 1)))) & 1u) != 0u;              \
                MF_UNROLL for (int i = 0; i < D; ++i) MF_UNROLL for (int jj = 0; jj <= i; ++jj)                       \
                    if (((i * D + jj) * S) / Cfg::StC::UNIT == HC::tail_unit(t))                                      \
                        C[i][jj] = got ? cv[t][(i * D + jj) - HC::tail_unit(t) * UEL] : C[i][jj];                     \
                MF_UNROLL for (int k = 0; k < UEL; ++k) cv[t][k] = rC.tail_at(t, k);                                  \
            }                                                                                                         \
        }                                                                                                             \
        MF_UNROLL for (int i = 0; i < D; ++i) mvec[i] = rb.at(i);                                                     \
        /* HREG: this step's row of H (pH is a row ahead by now), straight into hk; first used, behind a full drain, */ \
        /* in front of Obs::apply                                                                                    */ \
        if constexpr (Cfg::HREG) yreg_load(pH - M * D * S, eH, a.debug | ((a.debug >> 1) & 1), hvoff, hk);            \
        else { MF_UNROLL for (int i = 0; i < M * D; ++i) hk[i] = rH.at(i); }                                          \
        if constexpr (Cfg::YREG) {                                                                                    \
            /* this step's y out of the group; in the group's last step the next group is loaded over it */           \
            yk[0] = yr.q[0];                                                                                          \
            MF_UNROLL for (int g = 1; g < Cfg::YG; ++g) yk[0] = ((int)(j % Cfg::YG) == g) ? yr.q[g] : yk[0];          \
            /* (pins the compiler's own wait for the group's loads here, behind the drain above, not at y's first use) */ \
            asm volatile("" : "+v"(yk[0]));                                                                           \
            if (yfetch && more) yreg_load(py, ey, a.debug | ((a.debug >> 1) & 1), yr.voff, yr.q);                 \
        } else {                                                                                                      \
            MF_UNROLL for (int i = 0; i < M; ++i)                                                                     \
                yk[i] = *reinterpret_cast<const T*>(ry.row + ((int)(j % Cfg::YG) * M + i) * (int)sizeof(T));          \
        }                                                                                                             \
        if (RSTEP) { MF_UNROLL for (int i = 0; i < M * M; ++i) Rsh[i] = rR.at(i); }                                    \
        T Bm[D][D];                                                                                                   \
        MF_UNROLL for (int i = 0; i < D; ++i) MF_UNROLL for (int jj = 0; jj < D; ++jj) Bm[i][jj] = rA.at(i * D + jj); \
        if constexpr (NTA > 0) {                                                                                      \
            /* the head units that the NEXT row carries go from the tail slots, where this step's fetch left them, to  */ \
            /* the row's head slots, which are dead now: the fetch of the next row masks exactly those out and may    */ \
            /* refill the tail slots.  A unit that is not carried is written back to its own tail slot: no branch.    */ \
            /* (copied as values of T, the type the row was read with: the stores stay behind those reads)            */ \
            char* arow = smem + Cfg::OFF_A + lane * (Cfg::StA::U * Cfg::StA::UNIT);                                   \
            MF_UNROLL for (int t = 0; t < NTA; ++t) {                                                                 \
                const bool mv = MovedSchedule<typename Cfg::StA>::carried(dA.sch1, t, (unsigned)((j + 1) & (CPER - 1))); \
                const int src = (Cfg::StA::UB + t) * Cfg::StA::UNIT, dst = mv ? HCA::tail_unit(t) * Cfg::StA::UNIT : src; \
                T un[Cfg::StA::UNIT / S];                                                                             \
                MF_UNROLL for (int k = 0; k < Cfg::StA::UNIT / S; ++k) un[k] = *reinterpret_cast<const T*>(arow + src + k * S); \
                MF_UNROLL for (int k = 0; k < Cfg::StA::UNIT / S; ++k) *reinterpret_cast<T*>(arow + dst + k * S) = un[k]; \
            }                                                                                                         \
        }                                                                                                             \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                            \
        MF_CHECKSUM_ACC                                                                                               \
        MF_STAMP_AT(ts2)                                                                                              \
        const Pump pump{dA, dC, db, dH, dy, dR, make_srd(pA, eA, a.debug),                                            \
                        make_srd(pC, eC, a.debug | ((a.debug >> 2) & 1)),                                             \
                        make_srd(pb, eb, a.debug | ((a.debug >> 1) & 1)),                                             \
                        make_srd(pH, eH, a.debug | ((a.debug >> 1) & 1)),                                             \
                        make_srd(py, ey, a.debug | ((a.debug >> 1) & 1)),                                             \
                        make_srd(pR, eR, a.debug | ((a.debug >> 1) & 1)), lds0, more, yfetch,                         \
                        (unsigned)((j + 1) & (CPER - 1))};                                                            \
        MF_EXP_STEP_NEXT                                                                                              \
        MF_NOPUMP_ISSUE                                                                                               \
        const bool active = j < len;                                                                                  \
        kf_lds_step<T, D, M, SPIKE, FIRST>(E, laC, acc_yry, acc_ww, C, mvec, hk, yk, Rsh, Bm, pump, active, c > 0);    \
        if (E.bad && first_bad < 0) first_bad = tau0 + j;                                                             \
        if constexpr (Cfg::YREG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   /* (yreg_load) */                 \
        MF_STAMP_ACC                                                                                                  \
    }
    long j = 0;
    long first_bad = -1;          // the block whose elimination step first met a non-positive pivot
    if (nsteps > 0) MF_KF_LDS_STEP(true)
    for (j = 1; j < nsteps; ++j) MF_KF_LDS_STEP(false)
#undef MF_KF_LDS_STEP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (valid) {
        const T scalar = T(-0.5) * (acc_yry + acc_ww) + T(0.5) * E.quad - laC.value() - E.laL.value();
        store_chunk<T, D, SPIKE>(out, id, E, scalar);
        if (E.bad && a.info) raise_pivot(a.info, s * a.Tn + (first_bad < 0 ? tau0 : first_bad));
#ifdef MF_CHECKSUM
        out.GU[id * D * D + 0] = cs_A; out.GU[id * D * D + 1] = cs_C; out.GU[id * D * D + 2] = cs_b;
        out.gU[id * D + 0] = cs_H; out.gU[id * D + 1] = cs_y;
#endif
#ifdef MF_STAMP
        if (lane == 0) {   // diagnostic build only: overwrite this chunk's GU block with the stamp sums
            out.GU[id * D * D + 0] = (T)st_wait; out.GU[id * D * D + 1] = (T)st_io; out.GU[id * D * D + 2] = (T)st_comp;
        }
#endif
    }
}

}  // namespace mf
