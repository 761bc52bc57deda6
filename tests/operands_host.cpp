// Host-only pin of the operand binding (sputnik_amd/csrc/operands.cpp): for a
// fixed list of descriptors, the Status, the metadata flags and, when
// accepted, every non-zero GemmParams field of each of the six products in
// all four transposes. One line per case; tests/test_operands_host.py
// compares the output with tests/golden/operands.txt. Compiled together with
// operands.cpp; no libsputnik.so, no HIP runtime call. The descriptors hold
// fake, pairwise distinct addresses (operand A 0xa1.., B 0xb1.., C 0xc1..):
// nothing is dereferenced, and a swapped pointer shows in the output.
#include <cstdio>
#include <functional>
#include <string>

#include "api_internal.h"
#include "block_gemm.h"
#include "dispatch_internal.h"

using sputnik::block::BlockMatrix;
using sputnik::block::BlockSize;
using sputnik::block::Matrix;
using sputnik_amd::GemmParams;
using sputnik_amd::Status;

namespace {

enum Op { kDsd, kDds, kSdd, kSsd, kSds, kDss, kNumOps };
const char *const kOpNames[kNumOps] = {"dsd", "dds", "sdd", "ssd", "sds", "dss"};
// Which of A, B, C a product takes as a BCSR matrix.
const bool kSparse[kNumOps][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1},
                                  {1, 0, 1}, {0, 1, 1}, {1, 1, 0}};

const void *Fake(int operand, int field) {
  return reinterpret_cast<const void *>(
      static_cast<uintptr_t>(0xa0 + 0x10 * operand + field));
}

// Every operand as a BCSR descriptor; a dense one uses rows, cols and data.
struct Problem {
  Op op;
  bool ta, tb;
  BlockMatrix x[3];  // A, B, C
  bool sparse(int i) const { return kSparse[op][i]; }
  Matrix dense(int i) const { return Matrix(x[i].rows, x[i].cols, x[i].data); }
};

BlockMatrix Full(int operand, int rows, int cols) {
  BlockMatrix m(rows, cols, BlockSize::k128, 2 * 128 * 128, Fake(operand, 1),
                Fake(operand, 2), Fake(operand, 3), Fake(operand, 4),
                Fake(operand, 5), Fake(operand, 6), Fake(operand, 8));
  m.row_indices = const_cast<void *>(Fake(operand, 7));
  return m;
}

Problem Make(Op op, bool ta, bool tb, int m, int k, int n) {
  return Problem{op, ta, tb,
                 {ta ? Full(0, k, m) : Full(0, m, k),
                  tb ? Full(1, n, k) : Full(1, k, n), Full(2, m, n)}};
}

// The binding code under test.
sputnik_amd::Product Bind(const Problem &q) {
  using sputnik_amd::Operand;
  const Matrix dense[3] = {q.dense(0), q.dense(1), q.dense(2)};
  auto operand = [&](int i) { return q.sparse(i) ? Operand(q.x[i]) : Operand(dense[i]); };
  return sputnik_amd::Bind(operand(0), q.ta, operand(1), q.tb, operand(2));
}

const char *Name(Status st) {
  switch (st) {
    case Status::kOk: return "kOk";
    case Status::kNotSupported: return "kNotSupported";
    case Status::kNoKernel: return "kNoKernel";
    case Status::kMissingMetadata: return "kMissingMetadata";
    case Status::kMissingRowIndices: return "kMissingRowIndices";
  }
  return "?";
}

void Field(const char *name, const void *v) {
  if (v != nullptr) std::printf(" %s=%p", name, v);
}
void Field(const char *name, long long v) {
  if (v != 0) std::printf(" %s=%lld", name, v);
}
void Field(const char *name, unsigned v) { Field(name, (long long)v); }
void Field(const char *name, int v) { Field(name, (long long)v); }

// (a new GemmParams field needs a line below)
static_assert(sizeof(GemmParams) == 328, "GemmParams changed");
void Fields(const GemmParams &p) {
#define F(f) Field(#f, p.f)
  F(s_data); F(s_offsets); F(s_indices); F(s_block_offsets); F(s_ld);
  F(d_data); F(d_ld); F(c_data); F(c_ld); F(c_row_indices); F(c_offsets);
  F(c_indices); F(num_rows); F(num_jtiles); F(j_limit); F(k_limit);
  F(num_tiles); F(grid); F(persistent); F(tile_counter); F(pair);
  F(pair_partials); F(pair_flags); F(pair_epoch); F(pair_sync); F(pair_error);
  F(pair_fault); F(pair_xcd2); F(pair_split); F(split_bn); F(debug);
  F(d_offsets); F(d_indices); F(d_block_offsets); F(s_blocks); F(sdd_ksplit);
  F(ks_flags); F(sdd_order); F(tall_flush_w); F(tall_odd_share);
  F(min_handoff); F(xcd_rows); F(sdd_krot); F(sdd_spread); F(sdd_tail);
  F(tail_cus); F(z_data); F(act); F(u_data); F(du_data); F(bias);
#undef F
}

void Report(const std::string &name, const Problem &q) {
  const sputnik_amd::Product r = Bind(q);
  std::printf("%s.%c%c %s: %s meta=%d%d", kOpNames[q.op], q.ta ? 't' : 'n',
              q.tb ? 't' : 'n', name.c_str(), Name(r.status), r.s_meta, r.d_meta);
  if (r.status == Status::kOk) Fields(r.p);
  std::printf("\n");
}

using Edit = std::function<void(Problem &)>;
const char kLetter[3] = {'a', 'b', 'c'};

void NoBlocks(BlockMatrix &m) {
  m.nonzeros = 0;
  m.data = m.indices = nullptr;
}
void NoMeta(BlockMatrix &m) { m.offsets_t = m.indices_t = m.block_offsets = nullptr; }
void Block64(BlockMatrix &m) { m.block_size = BlockSize::k64; }
void NoRowIndices(BlockMatrix &m) { m.row_indices = nullptr; }
// C's columns, or B's k extent, grow by one unit of that extent.
void ShapeC(Problem &q) { q.x[2].cols += q.sparse(2) ? 128 : 8; }
void ShapeK(Problem &q) {
  (q.tb ? q.x[1].cols : q.x[1].rows) += q.sparse(1) || q.sparse(0) ? 128 : 8;
}

void Cases(Op op, bool ta, bool tb) {
  const bool *sp = kSparse[op];
  // m, k, n: 128-multiples where a BCSR operand has that extent, else ragged.
  const bool m_sp = sp[0] || sp[2], k_sp = sp[0] || sp[1], n_sp = sp[1] || sp[2];
  const int m = m_sp ? 256 : 72, k = k_sp ? 384 : 72, n = n_sp ? (m_sp ? 128 : 256) : 72;
  const Problem base = Make(op, ta, tb, m, k, n);
  auto run = [&](const std::string &name, const Problem &from, const Edit &e) {
    Problem q = from;
    e(q);
    Report(name, q);
  };
  auto each = [&](const std::string &name, bool want_sparse,
                  const std::function<void(Problem &, int)> &e, int first = 0,
                  int last = 2) {
    for (int i = first; i <= last; ++i)
      if (sp[i] == want_sparse)
        run(name + "_" + kLetter[i], base, [&](Problem &q) { e(q, i); });
  };

  run("ok", base, [](Problem &) {});
  // no transposed metadata on any operand
  run("no_meta", base, [](Problem &q) { for (auto &x : q.x) NoMeta(x); });
  each("empty", true, [](Problem &q, int i) { NoBlocks(q.x[i]); });
  // a zero extent: the dense operands it empties have null data, the sparse
  // ones no blocks
  for (int dim = 0; dim < 3; ++dim)
    run(std::string("zero_") + "mkn"[dim],
        Make(op, ta, tb, dim == 0 ? 0 : m, dim == 1 ? 0 : k, dim == 2 ? 0 : n), [](Problem &q) {
          for (int i = 0; i < 3; ++i)
            if ((long long)q.x[i].rows * q.x[i].cols == 0) {
              if (q.sparse(i)) NoBlocks(q.x[i]);
              else q.x[i].data = nullptr;
            }
        });
  each("no_offsets_t", true, [](Problem &q, int i) { q.x[i].offsets_t = nullptr; }, 0, 1);
  each("no_indices_t", true, [](Problem &q, int i) { q.x[i].indices_t = nullptr; }, 0, 1);
  each("no_block_offsets", true, [](Problem &q, int i) { q.x[i].block_offsets = nullptr; }, 0, 1);
  if (sp[2]) {
    run("no_row_indices", base, [](Problem &q) { NoRowIndices(q.x[2]); });
    run("no_row_indices_empty", base, [](Problem &q) {
      NoRowIndices(q.x[2]);
      NoBlocks(q.x[2]);
    });
  }
  each("b64", true, [](Problem &q, int i) { Block64(q.x[i]); });
  run("shape_c", base, ShapeC);
  run("shape_k", base, ShapeK);
  if (!m_sp) run("m12", Make(op, ta, tb, 12, k, n), [](Problem &) {});
  if (!k_sp) run("k12", Make(op, ta, tb, m, 12, n), [](Problem &) {});
  if (!n_sp) run("n12", Make(op, ta, tb, m, k, 12), [](Problem &) {});
  each("nnz", true, [](Problem &q, int i) { q.x[i].nonzeros += 64 * 64; });
  // 32767 and 32768 blocks along each extent a BCSR operand has
  for (int blocks : {32767, 32768}) {
    const std::string suffix = "_" + std::to_string(blocks) + "blocks";
    if (m_sp) run("m" + suffix, Make(op, ta, tb, blocks * 128, k, n), [](Problem &) {});
    if (k_sp) run("k" + suffix, Make(op, ta, tb, m, blocks * 128, n), [](Problem &) {});
    if (n_sp) run("n" + suffix, Make(op, ta, tb, m, k, blocks * 128), [](Problem &) {});
  }
  each("null_data", false, [](Problem &q, int i) { q.x[i].data = nullptr; });
  each("null_data", true, [](Problem &q, int i) { q.x[i].data = nullptr; });
  each("null_indices", true, [](Problem &q, int i) { q.x[i].indices = nullptr; });
  each("null_offsets", true, [](Problem &q, int i) { q.x[i].offsets = nullptr; });
  // The stride rule: rows of one DMA tile (64, 128 or the dense-output tile's
  // 512) x the leading dimension x 2 bytes against the 31-bit lane offset.
  // Both sides of each of the three limits, on the leading dimension of each
  // dense input, in that extent's granularity.
  for (int i = 0; i < 2; ++i) {
    if (sp[i]) continue;
    // lda = ta ? m : k, ldb = tb ? k : n
    const int which = i == 0 ? (ta ? 0 : 1) : (tb ? 1 : 2);
    const int gran = (which == 0 ? m_sp : which == 1 ? k_sp : n_sp) ? 128 : 8;
    for (int rows : {64, 128, 512})
      for (int over : {0, 1}) {
        const int ld = (int)(0x7fffffffLL / (2 * rows) / gran + over) * gran;
        run(std::string("ld") + kLetter[i] + "_" + std::to_string(ld),
            Make(op, ta, tb, which == 0 ? ld : m, which == 1 ? ld : k, which == 2 ? ld : n),
            [](Problem &) {});
      }
  }
  if (op == kDss)
    for (int kk : {32768, 32768 + 128})
      run("k" + std::to_string(kk), Make(op, ta, tb, m, kk, n), [](Problem &) {});

  // Precedence: two rules broken at once.
  each("b64+shape_c", true, [](Problem &q, int i) { Block64(q.x[i]); ShapeC(q); });
  each("b64+shape_k", true, [](Problem &q, int i) { Block64(q.x[i]); ShapeK(q); });
  each("no_meta+shape_c", true, [](Problem &q, int i) { NoMeta(q.x[i]); ShapeC(q); }, 0, 1);
  each("no_meta+null_data_c", true, [](Problem &q, int i) { NoMeta(q.x[i]); q.x[2].data = nullptr; }, 0, 1);
  if (sp[2]) {
    each("no_meta+b64_c", true, [](Problem &q, int i) { NoMeta(q.x[i]); Block64(q.x[2]); }, 0, 1);
    each("no_meta+no_row_indices_c", true,
         [](Problem &q, int i) { NoMeta(q.x[i]); NoRowIndices(q.x[2]); }, 0, 1);
    each("b64+b64_c", true, [](Problem &q, int i) { Block64(q.x[i]); Block64(q.x[2]); }, 0, 1);
    run("b64_c+no_row_indices", base, [](Problem &q) { Block64(q.x[2]); NoRowIndices(q.x[2]); });
    run("nnz_c+no_row_indices", base, [](Problem &q) { q.x[2].nonzeros += 64 * 64; NoRowIndices(q.x[2]); });
    run("shape_c+no_row_indices", base, [](Problem &q) { ShapeC(q); NoRowIndices(q.x[2]); });
    run("b64_c+null_data_a", base, [](Problem &q) { Block64(q.x[2]); q.x[0].data = nullptr; });
  }
  if (op == kDss) {
    run("no_meta_a+no_meta_b", base, [](Problem &q) { NoMeta(q.x[0]); NoMeta(q.x[1]); });
    run("b64_a+b64_b", base, [](Problem &q) { Block64(q.x[0]); Block64(q.x[1]); });
    run("no_meta_a+k32896", Make(op, ta, tb, m, 32768 + 128, n), [](Problem &q) { NoMeta(q.x[0]); });
  }
}

}  // namespace

int main() {
  for (int op = 0; op < kNumOps; ++op)
    for (int t = 0; t < 4; ++t) Cases(static_cast<Op>(op), t / 2 != 0, t % 2 != 0);
  return 0;
}
