// Host IPC reader under AddressSanitizer + UBSan (CPU build only: GPU sanitizers are not available on the pool).
// Builds the reader's host sources (tests/helpers.py: READER_HOST_SOURCES) with g++ (no HIP involved), then mutates the
// given fixture files the way tests/test_reader_fuzz.py does and drains them through IPCBufferStreamReader with and without
// projections.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include
//       tests/sanitize/fuzz_reader.cpp duckdb-arrow_amd/csrc/{ipc_format,io_pool,host_codec,frame_walk,batch_slice}.cpp
//       duckdb-arrow_amd/csrc/{ipc_stream_reader,c_stream}.cpp
//       -ldl -lpthread -o fuzz_reader && ./fuzz_reader ITERATIONS file...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../duckdb-arrow_amd/csrc/ipc_stream_reader.hpp"

using namespace miarrow;

// ---- the Arrow C stream export (c_stream.cpp) under the sanitizers: stubs for what c_api.cpp provides in the library
struct mi_reader {
  std::unique_ptr<IPCStreamReader> reader;
};
namespace miarrow {
std::unique_ptr<IPCStreamReader> TakeReader(mi_reader* r) { return std::move(r->reader); }
int WrapC(const std::function<void()>& f) {
  try {
    f();
    return 0;
  } catch (const std::exception&) {
    return 22;
  }
}
}  // namespace miarrow
extern "C" int mi_reader_export_stream(mi_reader* r, int32_t accept_dictionaries, struct ArrowArrayStream* out);

static void TouchArray(const ArrowArray* a, uint64_t* sum) {
  *sum += static_cast<uint64_t>(a->length + a->n_buffers);
  for (int64_t i = 0; i < a->n_children; i++) TouchArray(a->children[i], sum);
  if (a->dictionary) TouchArray(a->dictionary, sum);
}

static int DrainStream(const std::vector<uint8_t>& buf) {
  int batches = 0;
  try {
    std::vector<ArrowIPCBuffer> bufs;
    bufs.push_back(ArrowIPCBuffer{reinterpret_cast<uint64_t>(buf.data()), static_cast<uint64_t>(buf.size())});
    mi_reader r;
    r.reader = std::make_unique<IPCBufferStreamReader>(bufs);
    ArrowArrayStream st;
    if (mi_reader_export_stream(&r, 1, &st) != 0) return -1;
    ArrowSchema schema;
    if (st.get_schema(&st, &schema) == 0) schema.release(&schema);
    std::vector<ArrowArray> held;   // arrays may outlive the stream: released afterwards
    while (batches < 64) {
      ArrowArray a;
      if (st.get_next(&st, &a) != 0) { (void)st.get_last_error(&st); break; }
      if (!a.release) break;
      uint64_t sum = 0;
      TouchArray(&a, &sum);
      held.push_back(a);
      batches++;
    }
    st.release(&st);
    for (auto& a : held) a.release(&a);
  } catch (const std::exception&) {
    return -1;
  }
  return batches;
}

// What the K8 kernels compute from a deferred body (DecodedBatch::deferred: LZ4 frames still compressed, block tables built
// by the reader), restated serially with every access checked: the tables are the host half of the GPU decompressor.
static std::vector<uint8_t> DecodeDeferred(const DecodedBatch& b) {
  const DeferredBody& d = *b.deferred;
  std::vector<uint8_t> out(static_cast<size_t>(b.body_size), 0);
  auto need = [](bool ok) { if (!ok) throw std::runtime_error("deferred LZ4 body is malformed"); };
  for (auto& f : d.buffers) {
    need(f.comp_off >= 0 && f.comp_len >= 0 && f.comp_off + f.comp_len <= d.comp_size);
    need(f.out_off >= 0 && f.out_len >= 0 && f.out_off + f.out_len <= b.body_size);
    if (f.raw) {
      need(f.comp_len >= f.out_len);
      std::memcpy(out.data() + f.out_off, d.comp + f.comp_off, static_cast<size_t>(f.out_len));
      continue;
    }
    need(static_cast<size_t>(f.first_block) + f.n_blocks <= d.blocks.size());
    int64_t op = f.out_off;
    const int64_t out_end = f.out_off + f.out_len;
    for (uint32_t k = 0; k < f.n_blocks; k++) {
      const auto& blk = d.blocks[f.first_block + k];
      need(static_cast<int64_t>(blk.comp_off) >= f.comp_off && static_cast<int64_t>(blk.comp_off) + blk.comp_size <= f.comp_off + f.comp_len);
      const uint8_t* ip = d.comp + blk.comp_off;
      const uint8_t* const iend = ip + blk.comp_size;
      if (blk.stored) {
        need(op + blk.comp_size <= out_end);
        std::memcpy(out.data() + op, ip, blk.comp_size);
        op += blk.comp_size;
        continue;
      }
      while (ip < iend) {
        const uint32_t token = *ip++;
        uint64_t ll = token >> 4;
        if (ll == 15) {
          uint8_t x;
          do { need(ip < iend); x = *ip++; ll += x; } while (x == 255);
        }
        need(ll <= static_cast<uint64_t>(iend - ip) && op + static_cast<int64_t>(ll) <= out_end);
        std::memcpy(out.data() + op, ip, ll);
        ip += ll;
        op += static_cast<int64_t>(ll);
        if (ip >= iend) break;
        need(iend - ip >= 2);
        const uint32_t offset = ip[0] | (ip[1] << 8);
        ip += 2;
        uint64_t ml = token & 15;
        if (ml == 15) {
          uint8_t x;
          do { need(ip < iend); x = *ip++; ml += x; } while (x == 255);
        }
        ml += 4;
        need(offset != 0 && static_cast<int64_t>(offset) <= op - f.out_off && op + static_cast<int64_t>(ml) <= out_end);
        for (uint64_t i = 0; i < ml; i++, op++) out[static_cast<size_t>(op)] = out[static_cast<size_t>(op - offset)];
      }
    }
    need(op == out_end);
  }
  return out;
}

// An intact LZ4 stream read twice -- bodies decompressed by the reader (liblz4), and deferred + the restatement above:
// every buffer span must hold the same bytes.  Returns the number of record batches that were deferred.
static int CompareDeferredWithHost(const std::vector<uint8_t>& buf) {
  std::vector<ArrowIPCBuffer> bufs;
  bufs.push_back(ArrowIPCBuffer{reinterpret_cast<uint64_t>(buf.data()), static_cast<uint64_t>(buf.size())});
  IPCBufferStreamReader host(bufs), gpu(bufs);
  gpu.SetDeferLz4(true);
  DecodedBatch a, b;
  int deferred = 0;
  while (true) {
    const bool more_a = host.GetNextBatch(&a, true), more_b = gpu.GetNextBatch(&b, true);
    if (more_a != more_b) std::abort();
    if (!more_a) break;
    if (!b.deferred) continue;
    deferred++;
    const std::vector<uint8_t> body = DecodeDeferred(b);
    if (a.nodes.size() != b.nodes.size() || a.body_size != b.body_size) std::abort();
    for (size_t n = 0; n < a.nodes.size(); n++)
      for (size_t k = 0; k < a.nodes[n].spans.size(); k++) {
        const auto& x = a.nodes[n].spans[k];
        const auto& y = b.nodes[n].spans[k];
        if (x.length != y.length || x.offset != y.offset) std::abort();
        if (x.length > 0 && std::memcmp(a.body + x.offset, body.data() + y.offset, static_cast<size_t>(x.length)) != 0) std::abort();
      }
  }
  return deferred;
}

static int Drain(const std::vector<uint8_t>& buf, bool project, std::mt19937_64& rng) {
  int batches = 0;
  try {
    std::vector<ArrowIPCBuffer> bufs;
    bufs.push_back(ArrowIPCBuffer{reinterpret_cast<uint64_t>(buf.data()), static_cast<uint64_t>(buf.size())});
    IPCBufferStreamReader rd(bufs);
    rd.SetDeferLz4(rng() % 2 == 0);   // LZ4 bodies handed out compressed, with the block tables of the GPU decompressor
    rd.SetDeferZstd(rng() % 2 == 0);  // ZSTD bodies too: the host walk of frame / block / section headers (WalkZstdFrame)
    const ArrowSchemaModel& schema = rd.GetBaseSchema();
    {  // the flatbuffer builder under the sanitizers too: re-encode the schema, read it back, same top-level shape
      const std::vector<uint8_t> msg = EncodeSchemaMessage(schema);
      std::vector<ArrowIPCBuffer> again;
      again.push_back(ArrowIPCBuffer{reinterpret_cast<uint64_t>(msg.data()), static_cast<uint64_t>(msg.size())});
      IPCBufferStreamReader rd2(again);
      if (rd2.GetBaseSchema().fields.size() != schema.fields.size()) std::abort();
      std::vector<std::pair<int64_t, int64_t>> nodes(3, {5, 1});
      std::vector<mi_buffer_span> spans(7, mi_buffer_span{64, 8});
      const std::vector<uint8_t> rb = EncodeRecordBatchMessage(5, nodes, spans, 4096);
      if (rb.size() < 16) std::abort();
    }
    if (project && !schema.fields.empty()) {
      std::vector<std::string> names;
      for (auto& f : schema.fields)
        if (rng() % 2) names.push_back(f.name);
      if (names.empty()) names.push_back(schema.fields[0].name);
      rd.SetColumnProjection(names);
    }
    DecodedBatch b;
    while (batches < 64 && rd.GetNextBatch(&b, /*accept_dictionaries*/ true)) {
      batches++;
      // touch every byte the reader says belongs to a buffer
      uint64_t sum = 0;
      std::vector<uint8_t> expanded;
      const uint8_t* body = b.body;
      if (b.deferred && b.deferred->codec == 1) {
        // what the kernels rely on: every block, section and table source the walk names lies inside the body / the table
        const DeferredBody& d = *b.deferred;
        if (d.zblocks.size() != d.blocks.size()) std::abort();
        for (size_t i = 0; i < d.zblocks.size(); i++) {
          const zstd::BlockInfo& z = d.zblocks[i];
          if (static_cast<int64_t>(z.comp_off) + z.comp_size > d.comp_size) std::abort();
          if (z.huf_src > i || z.ll_src > i || z.of_src > i || z.ml_src > i) std::abort();
          if (z.type == 2 && (z.seq_pos + z.seq_hdr > z.comp_size || z.lit_hdr + z.lit_comp > z.comp_size)) std::abort();
          for (uint32_t k = 0; k < z.comp_size; k += 61) sum += d.comp[z.comp_off + k];
        }
        continue;
      }
      if (b.deferred) {
        try {
          expanded = DecodeDeferred(b);
        } catch (const std::runtime_error&) {
          continue;   // damaged block data: the device reports MI_ST_DECOMPRESS for it
        }
        body = expanded.data();
      }
      for (auto& nd : b.nodes)
        for (auto& sp : nd.spans)
          for (int64_t i = 0; i < sp.length; i += 61) sum += body[sp.offset + i];
      (void)sum;
    }
  } catch (const std::exception&) {
    return -1;
  }
  return batches;
}

// the file reader: footer index (IPC file format), header walk, partial projected preads, Seek
static int DrainFile(const std::vector<uint8_t>& buf, const std::string& tmp, bool project, std::mt19937_64& rng) {
  {
    std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
    out.write(reinterpret_cast<const char*>(buf.data()), static_cast<std::streamsize>(buf.size()));
  }
  int batches = 0;
  try {
    IPCFileStreamReader rd(tmp);
    const ArrowSchemaModel& schema = rd.GetBaseSchema();
    const auto& index = rd.BuildIndex();
    if (project && !schema.fields.empty()) {
      std::vector<std::string> names;
      for (auto& f : schema.fields)
        if (rng() % 2) names.push_back(f.name);
      if (names.empty()) names.push_back(schema.fields[0].name);
      rd.SetColumnProjection(names);
    }
    if (!index.empty() && rng() % 2) rd.Seek(index[rng() % index.size()].prefix_offset);
    DecodedBatch b;
    while (batches < 64 && rd.GetNextBatch(&b, true, /*skip_body*/ rng() % 5 == 0)) {
      batches++;
      uint64_t sum = 0;
      for (auto& nd : b.nodes)
        for (auto& sp : nd.spans)
          for (int64_t i = 0; i < sp.length; i += 61) sum += b.body[sp.offset + i];
      (void)sum;
    }
  } catch (const std::exception&) {
    return -1;
  }
  return batches;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s iterations file...\n", argv[0]);
    return 2;
  }
  const int iters = std::atoi(argv[1]);
  std::mt19937_64 rng(12345);
  long errors = 0, clean = 0, deferred_batches = 0;
  for (int a = 2; a < argc; a++) {
    std::ifstream in(argv[a], std::ios::binary);
    std::vector<uint8_t> src((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (src.empty()) continue;
    try {
      deferred_batches += CompareDeferredWithHost(src);
    } catch (const std::exception&) {
    }
    const size_t head = std::min<size_t>(src.size(), 1 << 16);
    for (int it = 0; it < iters; it++) {
      std::vector<uint8_t> buf = src;
      switch (it % 5) {
        case 4: {  // an extreme 64-bit word on an 8-byte boundary of the first 64 KB: Buffer{offset, length} and Block entries
                   // near INT64_MAX make `offset + length` wrap (random byte flips essentially never produce these)
          const uint64_t vals[] = {0x7FFFFFFFFFFFFFF8ull, 0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull, 0x4000000000000000ull,
                                   0xFFFFFFFFFFFFFFF8ull, 0x7FFFFFFFFFFFFE58ull};
          for (int k = 0; k < 2; k++) {
            const size_t p8 = (rng() % (head - 8)) & ~size_t(7);
            const uint64_t v = vals[rng() % 6];
            std::memcpy(&buf[p8], &v, 8);
          }
          break;
        }
        case 0:  // bytes in the first 64 KB (schema, first messages)
          for (int k = 0; k < 6; k++) buf[rng() % head] = static_cast<uint8_t>(rng());
          break;
        case 1: {  // an extreme 32-bit word somewhere in the first 64 KB
          const uint32_t vals[] = {0xFFFFFFFFu, 0u, 0x7FFFFFFFu, 0x80000000u, 0x7FFFFF00u};
          const size_t p = (rng() % (head - 4)) & ~size_t(3);
          const uint32_t v = vals[rng() % 5];
          std::memcpy(&buf[p], &v, 4);
          break;
        }
        case 2:  // truncation
          buf.resize(rng() % buf.size());
          break;
        default:  // bytes anywhere
          for (int k = 0; k < 8; k++) buf[rng() % buf.size()] = static_cast<uint8_t>(rng());
          break;
      }
      int r = Drain(buf, (it / 4) % 2 == 1, rng);
      if (it % 5 == 0) r = DrainStream(buf);
      if (it % 3 == 0) {
        const char* dir = std::getenv("TMPDIR");
        r = DrainFile(buf, std::string(dir ? dir : "/tmp") + "/mi_fuzz_reader.bin", (it / 3) % 2 == 1, rng);
      }
      if (r < 0) errors++; else clean++;
    }
  }
  std::printf("fuzz_reader: %ld clean, %ld rejected, %ld deferred LZ4 batches equal to the host decompressor, no sanitizer report\n", clean,
              errors, deferred_batches);
  return 0;
}
