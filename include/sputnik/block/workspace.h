// sputnik-amd: caller-owned workspaces for the transposed-B path. No
// counterpart in the reference, whose arguments.h hands every workspace to
// the caller through the descriptors; these give a caller bound to the fixed
// Matmul / MatmulEx signatures the same control.
//
// SDD NT / TT, and DSD NT over a nearly dense A, transpose B once into a
// scratch buffer when B is past the Infinity Cache and the product is dense
// enough. Without a registration that buffer is the
// library's: allocated inside the first such Matmul, grown (a stream
// synchronize and a free) when a larger B arrives, never used under graph
// capture. With memory registered for the stream, Matmul allocates, frees
// and synchronises nothing, and runs the same launches eagerly and captured.
#ifndef SPUTNIK_BLOCK_WORKSPACE_H_
#define SPUTNIK_BLOCK_WORKSPACE_H_

#include <cstddef>

#include "sputnik/block/arguments.h"

namespace sputnik {
namespace block {

// Registers `bytes` of device memory at `ptr` (16-byte aligned) as the
// transposed-B workspace of (current device, stream); ptr == nullptr
// unregisters. At most 16 registrations (hipErrorOutOfMemory beyond);
// hipErrorInvalidValue for a misaligned pointer, a zero size, or
// hipStreamPerThread. A stream with a registration never uses the
// library-owned buffer: memory too small for a product keeps that product on
// the NT / TT kernel.
//
// Lifetime: the memory must stay valid until all work enqueued with it has
// finished; for a launch captured into a graph, until the graph and every
// executable made from it are destroyed. A graph that captured it must not
// replay concurrently with other work that uses the same memory.
hipError_t SetStreamWorkspace(hipStream_t stream, void *ptr, size_t bytes);

// Bytes the transposed-B path would use for this problem under the current
// settings (a multiple of 256), 0 when the path does not apply. Host only.
size_t SddWorkspaceBytes(const Matrix a, bool transpose_a, const Matrix b,
                         bool transpose_b, const BlockMatrix c);
size_t DsdWorkspaceBytes(const BlockMatrix a, bool transpose_a, const Matrix b,
                         bool transpose_b, const Matrix c);

// Device memory the library holds on the current device (transposed-B
// buffers, pair-balancing workspaces, tile counters). Host only.
size_t RetainedBytes();

// Synchronises the current device, frees every library-owned transposed-B
// buffer on it and returns the bytes freed. A later Matmul without a
// registration allocates again.
size_t ReleaseWorkspaces();

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_WORKSPACE_H_
