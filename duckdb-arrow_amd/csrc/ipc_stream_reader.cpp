// ipc_stream_reader.cpp -- see ipc_stream_reader.hpp.
#include "ipc_stream_reader.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>

#include "host_codec.hpp"
#include "io_pool.hpp"

namespace miarrow {

// ------------------------------------------------------------------------------------------------ helpers
namespace {
struct SerializationException : std::runtime_error {
  SerializationException() : std::runtime_error("not enough data in file to deserialize result") {}
};

std::shared_ptr<void> DefaultBodyAlloc(size_t bytes, MessageType, uint8_t** ptr) {
  void* p = nullptr;
  if (posix_memalign(&p, 256, bytes ? bytes : 8) != 0 || p == nullptr) throw std::bad_alloc();
  *ptr = static_cast<uint8_t*>(p);
  return std::shared_ptr<void>(p, [](void* q) { std::free(q); });
}
}  // namespace

// ------------------------------------------------------------------------------------------------ base reader
const ArrowSchemaModel& IPCStreamReader::GetBaseSchema() {
  if (have_base_schema) return base_schema;
  ReadNextMessage({MessageType::SCHEMA}, /*end_of_stream_ok*/ false);
  base_schema = DecodeSchema(message_meta, message_meta_len);
  if (base_schema.features & (1u << 1)) {
    throw IOException("This stream uses unsupported feature DICTIONARY_REPLACEMENT");
  }
  // Big-endian streams (Schema.endianness = Big): metadata and message prefixes are little-endian whatever the producer,
  // only the buffers hold big-endian values.  The reference hands this to nanoarrow, which swaps while it decodes
  // (ArrowIpcDecoderSetEndianness, base_stream_reader.cpp:68-69); here the body of every message is swapped in place right
  // after it is read (SwapBodyEndianness), so that everything downstream -- kernels, C stream export, planner -- sees the
  // little-endian layout it expects.
  if (base_schema.endianness != 0 && base_schema.endianness != 1)
    throw IOException("Unknown Schema.endianness " + std::to_string(base_schema.endianness));
  have_base_schema = true;
  return base_schema;
}

const ArrowSchemaModel& IPCStreamReader::GetOutputSchema() {
  if (HasProjection()) return projected_schema;
  return GetBaseSchema();
}

// Projection pushdown by column name (the seam of base_stream_reader.cpp:146-212; error texts are the reference's).
// Names are the deduplicated top-level names; a name that two columns still share after deduplication cannot be
// addressed.  Per projected column the reader keeps its top-level index.
void IPCStreamReader::SetColumnProjection(const std::vector<std::string>& column_names) {
  if (column_names.empty()) throw InternalException("Can't request zero fields projected from IpcStreamReader");
  GetBaseSchema();
  const size_t n_top = base_schema.fields.size();
  std::vector<std::string> names(n_top);
  for (size_t i = 0; i < n_top; i++) names[i] = base_schema.fields[i].name;
  DeduplicateColumns(names);
  auto locate = [&](const std::string& wanted) -> size_t {
    size_t hit = n_top, hits = 0;
    for (size_t i = 0; i < n_top; i++) {
      if (names[i] != wanted) continue;
      if (hits++ == 0) hit = i;
    }
    if (hits > 1) throw InternalException("Field '" + wanted + "' refers to a duplicate column name in IPC file schema");
    if (hits == 0) throw InternalException("Field '" + wanted + "' does not exist in IPC file schema");
    return hit;
  };
  ArrowSchemaModel picked;
  picked.endianness = base_schema.endianness;
  picked.metadata = base_schema.metadata;
  std::vector<int32_t> top;
  for (const std::string& wanted : column_names) {
    const size_t i = locate(wanted);
    top.push_back(static_cast<int32_t>(i));
    picked.fields.push_back(base_schema.fields[i]);
  }
  // nothing changes unless every name resolved
  projected_columns.swap(top);
  projected_schema = std::move(picked);
}

// The prefix has been read into message_prefix: header (flatbuffer) next, then the body.  UNINITIALIZED = the
// end-of-stream marker.  (The reference splits this into DecodeMetadata + DecodeMessage, base_stream_reader.cpp:214-236;
// its BSWAP of the length only happens on big-endian hosts, which gfx950 hosts are not.)
MessageType IPCStreamReader::FinishMessage() {
  const int64_t metadata_size = message_prefix.metadata_size;
  if (metadata_size < 0) throw IOException("Expected metadata size >= 0 but got " + std::to_string(metadata_size));
  const bool end_of_stream = DecodeHeader(static_cast<idx_t>(metadata_size) + sizeof(message_prefix));
  if (end_of_stream) return MessageType::UNINITIALIZED;
  DecodeBody();
  return message.type;
}

bool IPCStreamReader::ParseHeader(const uint8_t* header_with_prefix, idx_t size) {
  // ArrowIpcDecoderDecodeHeader: metadata size 0 is the end-of-stream marker => ENODATA
  if (message_prefix.metadata_size == 0) return false;
  message_meta = header_with_prefix + sizeof(message_prefix);
  message_meta_len = static_cast<int64_t>(size - sizeof(message_prefix));
  message = DecodeMessageHeader(message_meta, message_meta_len);
  return true;
}

MessageType IPCStreamReader::ReadNextMessage(std::vector<MessageType> expected_types, bool end_of_stream_ok) {
  const MessageType got = ReadNextMessage();
  const bool at_end = got == MessageType::UNINITIALIZED;
  if (at_end && end_of_stream_ok) return got;
  if (std::find(expected_types.begin(), expected_types.end(), got) != expected_types.end()) return got;
  std::string wanted;
  for (MessageType t : expected_types) {
    if (!wanted.empty()) wanted += " or ";
    wanted += MessageTypeString(t);
  }
  throw IOException("Expected " + wanted + " Arrow IPC message but got " + (at_end ? "end of stream" : MessageTypeString(got)));
}

static bool HasUnionField(const ArrowField& f);

bool IPCStreamReader::GetNextBatch(DecodedBatch* out, bool accept_dictionaries, bool skip_body) {
  GetBaseSchema();
  std::vector<MessageType> expected = {MessageType::RECORD_BATCH};
  if (accept_dictionaries) expected.push_back(MessageType::DICTIONARY_BATCH);
  skip_record_batch_body = skip_body;
  MessageType message_type;
  try {
    message_type = ReadNextMessage(expected);
  } catch (...) {
    skip_record_batch_body = false;
    throw;
  }
  skip_record_batch_body = false;
  if (message_type == MessageType::UNINITIALIZED) return false;
  RecordBatchMeta meta = DecodeRecordBatch(message_meta, message_meta_len);
  if (skip_body && message_type == MessageType::RECORD_BATCH) {
    *out = DecodedBatch();
    out->length = meta.length;
    out->body_file_offset = cur_body_offset;
    out->compression = meta.compression;
    return true;
  }
  // before V5 a union owned a validity buffer of its own: the buffer walk (ArrowField::Layout) knows the V5 layout only
  if (message.version < 4 && !meta.is_dictionary)
    if (const ArrowField* u = WantedFieldWith(HasUnionField))
      throw NotImplementedException("Column '" + u->name + "': union arrays of a stream whose metadata version is below V5 carry a validity buffer and are not read");
  std::shared_ptr<const DeferredBody> deferred;
  if (meta.compression != -1 && cur_size > 0) deferred = DecompressBody(&meta);
  if (base_schema.endianness == 1) SwapBodyEndianness(meta);
  SliceBatch(base_schema, projected_columns, meta, cur_ptr, cur_size, cur_body_offset, cur_owner, out);
  if (deferred) {
    out->deferred = std::move(deferred);
    out->body = nullptr;
    out->compression = 0;
  }
  return true;
}

// Body compression (Message.fbs BodyCompression, method BUFFER): every buffer is `int64 uncompressed_length` (-1 = the
// bytes that follow are stored raw) + one frame.
std::shared_ptr<const DeferredBody> IPCStreamReader::DecompressBody(RecordBatchMeta* meta) {
  if (meta->compression != 0 && meta->compression != 1) throw IOException("Unknown BodyCompression codec " + std::to_string(meta->compression));
  const bool lz4 = meta->compression == 0;
  if (lz4 && !HostCodecAvailable(0))
    throw NotImplementedException("LZ4_FRAME compressed IPC body but liblz4.so.1 is not available on this host (the reference registers a ZSTD decompressor only)");
  if (!lz4 && !HostCodecAvailable(1)) throw NotImplementedException("ZSTD compressed IPC body but libzstd.so.1 is not available on this host");
  const DecompressedLayout lay = LayOutDecompressedBody(base_schema, projected_columns, meta, cur_ptr, cur_size, lz4 ? nullptr : &ZstdFrameContentSize);
  const size_t nbuf = meta->buffers.size();
  // GPU consumers (SetDeferLz4 / SetDeferZstd): keep the body compressed and hand out the frame / block tables instead
  if ((lz4 ? defer_lz4 : defer_zstd) && MayStayCompressed(base_schema, projected_columns, *meta, lay.total, cur_size)) {
    auto d = std::make_shared<DeferredBody>();
    d->comp = cur_ptr;
    d->comp_size = cur_size;
    d->codec = meta->compression;
    bool ok = true;
    for (size_t i = 0; i < nbuf && ok; i++) {
      const mi_buffer_span& b = meta->buffers[i];
      if (b.length == 0 || lay.ulen[i] == 0) continue;
      DeferredBody::Buffer f;
      int64_t declared;
      std::memcpy(&declared, cur_ptr + b.offset, 8);
      f.raw = declared == -1;
      f.comp_off = b.offset + 8;
      f.comp_len = b.length - 8;
      f.out_off = lay.opos[i];
      f.out_len = lay.ulen[i];
      if (!f.raw)
        ok = lz4 ? WalkLz4Frame(cur_ptr, f.comp_off, f.comp_len, static_cast<uint32_t>(d->buffers.size()), &f, &d->blocks)
                 : WalkZstdFrame(cur_ptr, f.comp_off, f.comp_len, static_cast<uint32_t>(d->buffers.size()), lay.ulen[i], &f, &d->blocks,
                                 &d->zblocks, &d->literal_scratch);
      d->buffers.push_back(f);
    }
    if (ok) {
      for (size_t i = 0; i < nbuf; i++) {
        mi_buffer_span& b = meta->buffers[i];
        b.offset = lay.opos[i];
        b.length = (b.length == 0) ? 0 : lay.ulen[i];
      }
      cur_size = lay.total;      // SliceBatch checks the spans against the decompressed layout; it never reads the body
      meta->compression = -1;
      return d;
    }
  }
  uint8_t* out = nullptr;
  std::shared_ptr<void> owner = body_allocator ? body_allocator(static_cast<size_t>(lay.total + 64), message.type, &out)
                                               : DefaultBodyAlloc(static_cast<size_t>(lay.total + 64), message.type, &out);
  // one frame per buffer, independent of each other -> the I/O pool's threads share them
  const uint8_t* in = cur_ptr;
  const int32_t codec = meta->compression;
  ParallelFor(static_cast<int>(nbuf), [&](int bi) {
    const size_t i = static_cast<size_t>(bi);
    mi_buffer_span& b = meta->buffers[i];
    if (b.length == 0) {
      b.offset = lay.opos[i];
      return;
    }
    const uint8_t* src = in + b.offset;
    int64_t declared;
    std::memcpy(&declared, src, 8);
    const int64_t n = lay.ulen[i];
    uint8_t* dst = out + lay.opos[i];
    if (declared == -1) std::memcpy(dst, src + 8, static_cast<size_t>(n));
    else HostDecompressFrame(codec, dst, n, src + 8, b.length - 8);
    const int64_t padded = (n + 63) & ~static_cast<int64_t>(63);
    std::memset(dst + n, 0, static_cast<size_t>(padded - n));
    b.offset = lay.opos[i];
    b.length = n;
  });
  compressed_owner = cur_owner;  // released with the next message
  cur_owner = owner;
  cur_ptr = out;
  cur_size = lay.total;
  meta->compression = -1;
  return nullptr;
}

static bool HasRunEndField(const ArrowField& f) {
  return f.type == MI_AT_RUN_END || std::any_of(f.children.begin(), f.children.end(), HasRunEndField);
}

static bool HasUnionField(const ArrowField& f) {
  return (f.type == MI_AT_UNION && !f.has_dictionary) || std::any_of(f.children.begin(), f.children.end(), HasUnionField);
}

// the first projected (or any, without a projection) top-level field that `has` something, or nullptr
const ArrowField* IPCStreamReader::WantedFieldWith(bool (*has)(const ArrowField&)) const {
  for (size_t i = 0; i < base_schema.fields.size(); i++) {
    const bool wanted = !HasProjection() || std::find(projected_columns.begin(), projected_columns.end(), static_cast<int32_t>(i)) != projected_columns.end();
    if (wanted && has(base_schema.fields[i])) return &base_schema.fields[i];
  }
  return nullptr;
}

void IPCStreamReader::SwapBodyEndianness(const RecordBatchMeta& meta) {
  // the swap itself would be right (run_ends is an int child), but no test pins big-endian run-end encoded columns yet
  for (size_t i = 0; i < base_schema.fields.size(); i++) {
    const bool wanted = !HasProjection() || std::find(projected_columns.begin(), projected_columns.end(), static_cast<int32_t>(i)) != projected_columns.end();
    if (wanted && !meta.is_dictionary && HasRunEndField(base_schema.fields[i]))
      throw NotImplementedException("Column '" + base_schema.fields[i].name + "': run-end encoded arrays in a big-endian stream are not read");
  }
  // ... and the same goes for unions (the offsets of a dense union are int32 and would be swapped)
  if (!meta.is_dictionary)
    if (const ArrowField* u = WantedFieldWith(HasUnionField))
      throw NotImplementedException("Column '" + u->name + "': union arrays in a big-endian stream are not read");
  if (cur_size <= 0) return;
  // the body must be ours to rewrite: caller-owned buffers (scan_arrow_ipc) are copied first
  if (!cur_owner) {
    uint8_t* copy = nullptr;
    cur_owner = DefaultBodyAlloc(static_cast<size_t>(cur_size) + 64, message.type, &copy);
    std::memcpy(copy, cur_ptr, static_cast<size_t>(cur_size));
    cur_ptr = copy;
  }
  SwapBody(base_schema, meta, NeededBuffers(base_schema, projected_columns, meta), const_cast<uint8_t*>(cur_ptr), cur_size);
}

// ------------------------------------------------------------------------------------------------ file reader

IPCFileStreamReader::IPCFileStreamReader(const std::string& path_p) : path(path_p) {
  fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) {
    throw IOException("Cannot open file \"" + path + "\": " + std::strerror(errno));
  }
  struct stat st;
  if (fstat(fd, &st) != 0) {
    ::close(fd);
    fd = -1;
    throw IOException("Cannot stat file \"" + path + "\": " + std::strerror(errno));
  }
  file_size = st.st_size;
}

IPCFileStreamReader::~IPCFileStreamReader() {
  if (fd >= 0) ::close(fd);
}

double IPCFileStreamReader::GetProgress() {
  if (file_size == 0) return 100;
  return (static_cast<double>(offset) / static_cast<double>(file_size)) * 100;
}

const uint8_t* IPCFileStreamReader::ReadData(uint8_t* ptr, idx_t size) {
  // BufferedFileReader::ReadData throws SerializationException when the file ends early
  constexpr idx_t kSlice = 256u << 10;  // smallest piece worth a thread hand-off
  if (size >= 4 * kSlice && IoThreads() > 1) {
    if (!SpanInside(offset, static_cast<int64_t>(size), file_size)) throw SerializationException();
    const int n = static_cast<int>(std::min<idx_t>((size + kSlice - 1) / kSlice, static_cast<idx_t>(2 * IoThreads())));
    const idx_t per = ((size + n - 1) / n + 4095) & ~static_cast<idx_t>(4095);
    const int64_t base = offset;
    ParallelFor(n, [&](int i) {
      idx_t lo = static_cast<idx_t>(i) * per, hi = std::min(size, lo + per);
      while (lo < hi) {
        ssize_t r = ::pread(fd, ptr + lo, hi - lo, static_cast<off_t>(base + static_cast<int64_t>(lo)));
        if (r < 0) {
          if (errno == EINTR) continue;
          throw IOException("Could not read from file \"" + path + "\": " + std::strerror(errno));
        }
        if (r == 0) throw SerializationException();
        lo += static_cast<idx_t>(r);
      }
    });
    offset += static_cast<int64_t>(size);
    return ptr;
  }
  idx_t done = 0;
  while (done < size) {
    ssize_t r = ::pread(fd, ptr + done, size - done, static_cast<off_t>(offset + static_cast<int64_t>(done)));
    if (r < 0) {
      if (errno == EINTR) continue;
      throw IOException("Could not read from file \"" + path + "\": " + std::strerror(errno));
    }
    if (r == 0) throw SerializationException();
    done += static_cast<idx_t>(r);
  }
  offset += static_cast<int64_t>(size);
  return ptr;
}

// Positions the reader on the next 8-byte boundary and reads one message prefix.  false = the file ends before a whole
// prefix could be read, which the reference treats as a clean end of stream (its aligned read throws
// SerializationException, ipc_file_stream_reader.cpp:103-129); the file size is known here, so no read is attempted.
bool IPCFileStreamReader::ReadPrefix() {
  const int64_t at = (offset + 7) & ~static_cast<int64_t>(7);
  if (at > file_size || file_size - at < static_cast<int64_t>(sizeof(message_prefix))) return false;
  offset = at;
  ReadData(reinterpret_cast<uint8_t*>(&message_prefix), sizeof(message_prefix));
  return true;
}

void IPCFileStreamReader::SkipBodyPadding() { offset = std::min(file_size, (offset + 7) & ~static_cast<int64_t>(7)); }

MessageType IPCFileStreamReader::ReadNextMessage() {
  static const char kFileMagic[8] = {'A', 'R', 'R', 'O', 'W', '1', 0, 0};
  while (!finished) {
    try {
      if (!ReadPrefix()) break;
    } catch (SerializationException&) {
      break;  // the file shrank under us: same outcome
    }
    // Arrow *file* format: the first 8 bytes are the magic, then comes an ordinary stream (ipc_file_stream_reader.cpp:107-119)
    if (offset == 8 && std::memcmp(kFileMagic, &message_prefix, 8) == 0) continue;
    if (message_prefix.continuation_token != kContinuationToken)
      throw IOException("Expected continuation token (0xFFFFFFFF) but got " + std::to_string(message_prefix.continuation_token));
    try {
      return FinishMessage();
    } catch (SerializationException& e) {
      throw IOException(std::string("SerializationException: ") + e.what());
    }
  }
  finished = true;
  return MessageType::UNINITIALIZED;
}

bool IPCFileStreamReader::DecodeHeader(const idx_t message_header_size) {
  // sizes come from the file: nothing is allocated for bytes the file cannot hold (BufferedFileReader::ReadData's
  // "not enough data in file to deserialize result")
  if (!SpanInside(offset, static_cast<int64_t>(message_prefix.metadata_size), file_size)) throw SerializationException();
  if (message_header.size() < message_header_size) message_header.resize(message_header_size);
  std::memcpy(message_header.data(), &message_prefix, sizeof(message_prefix));
  ReadData(message_header.data() + sizeof(message_prefix), static_cast<idx_t>(message_prefix.metadata_size));
  if (!ParseHeader(message_header.data(), message_header_size)) {
    finished = true;
    return true;
  }
  return false;
}

void IPCFileStreamReader::DecodeBody() {
  cur_owner.reset();
  cur_ptr = nullptr;
  cur_size = 0;
  if (message.body_length > 0) {
    SkipBodyPadding();
    cur_body_offset = offset;
    if (message.body_length > file_size - offset) throw SerializationException();  // before anything is allocated for it
    if (skip_record_batch_body && message.type == MessageType::RECORD_BATCH) {
      offset += message.body_length;  // step over the body without reading it
      return;
    }
    uint8_t* p = nullptr;
    bool compressed = false, stays_compressed = false;
    std::vector<std::pair<int64_t, int64_t>> ranges;
    if (message.type == MessageType::RECORD_BATCH || message.type == MessageType::DICTIONARY_BATCH) {
      const RecordBatchMeta meta = DecodeRecordBatch(message_meta, message_meta_len);
      compressed = meta.compression != -1;
      stays_compressed = ((defer_lz4 && meta.compression == 0) || (defer_zstd && meta.compression == 1)) && message.type == MessageType::RECORD_BATCH && base_schema.endianness == 0;
      // projection pushdown reaches the file: only the buffers of the projected columns are read (the reference reads
      // the whole body, ipc_file_stream_reader.cpp:71-89); what is skipped is never looked at
      if (message.type == MessageType::RECORD_BATCH) ranges = ProjectedBodyRanges(base_schema, projected_columns, meta, message.body_length, 256 << 10);
    }
    // uncompressed bodies, and LZ4 bodies a GPU consumer decompresses itself, are copied to the device as they are: they
    // go where the consumer wants them (pinned staging); bodies the host decompresses only need to be readable here
    const bool to_device = !compressed || stays_compressed;
    cur_owner = (body_allocator && to_device) ? body_allocator(static_cast<size_t>(message.body_length), message.type, &p)
                                              : DefaultBodyAlloc(static_cast<size_t>(message.body_length), message.type, &p);
    if (ranges.empty()) {
      ReadData(p, static_cast<idx_t>(message.body_length));
    } else {
      if (!SpanInside(offset, message.body_length, file_size)) throw SerializationException();
      const int64_t body0 = offset;
      for (auto& r : ranges) {
        if (r.second <= r.first) continue;
        offset = body0 + r.first;
        ReadData(p + r.first, static_cast<idx_t>(r.second - r.first));
      }
      offset = body0 + message.body_length;
    }
    cur_ptr = p;
    cur_size = message.body_length;
  } else {
    cur_body_offset = offset;
  }
}

void IPCFileStreamReader::Seek(int64_t prefix_offset) {
  offset = prefix_offset;
  finished = false;
}

bool IPCFileStreamReader::IndexFromFooter() {
  // Arrow IPC *file*: "ARROW1\0\0" stream footer int32 footer_len "ARROW1".  The footer lists every dictionary and
  // record-batch block {offset, metaDataLength, bodyLength}: random access for sharding without walking the headers
  // (the reference notes this as future work: ipc_file_stream_reader.cpp:113-115, arrow_file_scan.cpp:36-40).
  if (file_size < 8 + 10) return false;
  uint8_t magic[8];
  if (::pread(fd, magic, 8, 0) != 8 || std::memcmp(magic, "ARROW1\0\0", 8) != 0) return false;
  uint8_t tail10[10];
  if (::pread(fd, tail10, 10, static_cast<off_t>(file_size - 10)) != 10 || std::memcmp(tail10 + 4, "ARROW1", 6) != 0) return false;
  int32_t flen;
  std::memcpy(&flen, tail10, 4);
  if (flen <= 0 || static_cast<int64_t>(flen) + 18 > file_size) return false;
  std::vector<uint8_t> tail(static_cast<size_t>(flen) + 10);
  if (::pread(fd, tail.data(), tail.size(), static_cast<off_t>(file_size - static_cast<int64_t>(tail.size()))) != static_cast<ssize_t>(tail.size()))
    return false;
  std::vector<FooterBlock> dict_blocks, batch_blocks;
  if (!DecodeFooter(tail.data(), static_cast<int64_t>(tail.size()), file_size, &dict_blocks, &batch_blocks)) return false;
  std::vector<uint8_t> meta;
  auto add = [&](const FooterBlock& b, MessageType type) {
    // block.metaDataLength covers the 8-byte prefix + the padded flatbuffer
    if (b.offset < 8 || b.meta_len < 8 || !SpanInside(b.offset, b.meta_len, file_size) || !SpanInside(b.offset + b.meta_len, b.body_len, file_size))
      throw IOException("Footer block out of bounds");
    BatchIndexEntry e{b.offset, b.meta_len - 8, static_cast<int32_t>(type), b.offset + b.meta_len, b.body_len, 0};
    meta.resize(static_cast<size_t>(b.meta_len - 8));
    if (::pread(fd, meta.data(), meta.size(), static_cast<off_t>(b.offset + 8)) != static_cast<ssize_t>(meta.size()))
      throw IOException("Could not read record batch metadata at offset " + std::to_string(b.offset));
    e.n_rows = DecodeRecordBatch(meta.data(), static_cast<int64_t>(meta.size())).length;
    index.push_back(e);
  };
  // stream order: dictionaries precede the batches that use them
  std::vector<std::pair<FooterBlock, MessageType>> all;
  for (auto& b : dict_blocks) all.emplace_back(b, MessageType::DICTIONARY_BATCH);
  for (auto& b : batch_blocks) all.emplace_back(b, MessageType::RECORD_BATCH);
  std::sort(all.begin(), all.end(), [](const auto& x, const auto& y) { return x.first.offset < y.first.offset; });
  for (auto& b : all)
    if (b.first.offset >= offset) add(b.first, b.second);
  return true;
}

const std::vector<BatchIndexEntry>& IPCFileStreamReader::BuildIndex() {
  if (index_built) return index;
  GetBaseSchema();
  if (IndexFromFooter()) {
    index_built = true;
    return index;
  }
  index.clear();
  int64_t saved = offset;
  bool saved_finished = finished;
  // Walk headers only; bodies are skipped (the stream format has no footer index: SURVEY "Hard parts")
  std::vector<uint8_t> meta;
  int64_t pos = offset;
  while (true) {
    pos = (pos + 7) & ~static_cast<int64_t>(7);
    if (pos + 8 > file_size) break;
    ArrowIpcMessagePrefix p;
    offset = pos;
    try {
      ReadData(reinterpret_cast<uint8_t*>(&p), 8);
    } catch (SerializationException&) { break; }
    if (p.continuation_token != kContinuationToken || p.metadata_size <= 0) break;
    if (!SpanInside(pos + 8, p.metadata_size, file_size)) break;
    meta.resize(static_cast<size_t>(p.metadata_size));
    ReadData(meta.data(), static_cast<idx_t>(p.metadata_size));
    MessageHeader h = DecodeMessageHeader(meta.data(), p.metadata_size);
    BatchIndexEntry e{pos, p.metadata_size, static_cast<int32_t>(h.type), 0, h.body_length, 0};
    int64_t body = (offset + 7) & ~static_cast<int64_t>(7);
    e.body_offset = body;
    if (!SpanInside(body, h.body_length, file_size)) break;
    if (h.type == MessageType::RECORD_BATCH || h.type == MessageType::DICTIONARY_BATCH)
      e.n_rows = DecodeRecordBatch(meta.data(), p.metadata_size).length;
    index.push_back(e);
    pos = body + h.body_length;
  }
  offset = saved;
  finished = saved_finished;
  index_built = true;
  return index;
}

// ------------------------------------------------------------------------------------------------ buffer reader
IPCBufferStreamReader::IPCBufferStreamReader(std::vector<ArrowIPCBuffer> buffers_p) : buffers(std::move(buffers_p)) {}

// The caller's buffers are read in place (ipc_buffer_stream_reader.cpp:36-41: a pointer bump): `view` is the window over the
// buffer being consumed, `view_index` its place in the list; a buffer is opened when the first byte of it is asked for.
bool IPCBufferStreamReader::SeekUnreadByte() {
  while (!view.opened || view.pos >= view.size) {
    const idx_t next = view.opened ? view_index + 1 : view_index;
    if (next >= buffers.size()) return false;
    view_index = next;
    view.opened = true;
    view.ptr = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(buffers[next].ptr));
    view.size = static_cast<int64_t>(buffers[next].size);
    view.pos = 0;
    if (!view.ptr && view.size > 0) throw IOException("Arrow IPC buffer " + std::to_string(next) + " is a NULL pointer");
  }
  return true;
}

const uint8_t* IPCBufferStreamReader::ReadData(idx_t size) {
  // the reference only asserts (ipc_buffer_stream_reader.cpp:37); a short buffer is reported instead of read past
  if (!SpanInside(view.pos, static_cast<int64_t>(size), view.size)) {
    throw IOException("Unexpected end of Arrow IPC buffer: need " + std::to_string(size) + " bytes at position " +
                      std::to_string(view.pos) + " of " + std::to_string(view.size));
  }
  const uint8_t* p = view.ptr + view.pos;
  view.pos += static_cast<int64_t>(size);
  return p;
}

MessageType IPCBufferStreamReader::ReadNextMessage() {
  while (!finished && SeekUnreadByte()) {
    prefix_at = ReadData(sizeof(message_prefix));
    std::memcpy(&message_prefix, prefix_at, sizeof(message_prefix));
    // An IPC *file* handed over as a buffer begins with the magic the file reader steps over
    // (ipc_file_stream_reader.cpp:116-119); the reference's buffer reader has no such case, accepting it is a superset
    const bool file_magic = view_index == 0 && view.pos == 8 && std::memcmp("ARROW1\0\0", prefix_at, 8) == 0;
    if (file_magic) continue;
    if (message_prefix.continuation_token != kContinuationToken)
      throw IOException("Expected continuation token (0xFFFFFFFF) but got " + std::to_string(message_prefix.continuation_token));
    return FinishMessage();
  }
  finished = true;   // every buffer is consumed (or the end-of-stream marker was seen before)
  return MessageType::UNINITIALIZED;
}

bool IPCBufferStreamReader::DecodeHeader(idx_t message_header_size) {
  // the decoder wants prefix + metadata as one span: the metadata follows the prefix in the caller's buffer, so the span
  // starts where the prefix was read
  (void)ReadData(static_cast<idx_t>(message_prefix.metadata_size));
  const bool end_of_stream = !ParseHeader(prefix_at, message_header_size);
  if (end_of_stream) finished = true;
  return end_of_stream;
}

void IPCBufferStreamReader::DecodeBody() {
  cur_owner.reset();
  if (message.body_length > 0) {
    // bodies are 8-byte aligned relative to the start of the stream
    int64_t aligned = (view.pos + 7) & ~static_cast<int64_t>(7);
    if (aligned != view.pos) ReadData(static_cast<idx_t>(aligned - view.pos));
    cur_body_offset = view.pos;
    cur_ptr = ReadData(static_cast<idx_t>(message.body_length));
    cur_size = message.body_length;
  } else {
    cur_body_offset = view.pos;
    cur_ptr = nullptr;
    cur_size = 0;
  }
}

double IPCBufferStreamReader::GetProgress() {
  if (buffers.empty()) return 100;
  double done = static_cast<double>(view_index);
  if (view.size > 0 && view_index < buffers.size()) done += static_cast<double>(view.pos) / static_cast<double>(view.size);
  return std::min(100.0, 100.0 * done / static_cast<double>(buffers.size()));
}

const std::vector<BatchIndexEntry>& IPCBufferStreamReader::BuildIndex() {
  if (index_built) return index;
  GetBaseSchema();
  // header walk over every buffer from the current position, without touching reader state
  int64_t global_base = 0;
  for (idx_t b = 0; b < buffers.size(); b++) {
    const uint8_t* base = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(buffers[b].ptr));
    int64_t size = static_cast<int64_t>(buffers[b].size);
    int64_t pos = 0;
    if (view.opened && b < view_index) { global_base += size; continue; }
    if (b == view_index && view.opened) pos = view.pos;
    if (pos == 0 && b == 0 && size >= 8 && std::memcmp("ARROW1\0\0", base, 8) == 0) pos = 8;
    while (pos + 8 <= size) {
      ArrowIpcMessagePrefix p;
      std::memcpy(&p, base + pos, 8);
      if (p.continuation_token != kContinuationToken || p.metadata_size <= 0) break;
      if (!SpanInside(pos + 8, p.metadata_size, size)) break;
      MessageHeader h = DecodeMessageHeader(base + pos + 8, p.metadata_size);
      int64_t body = (pos + 8 + p.metadata_size + 7) & ~static_cast<int64_t>(7);
      if (!SpanInside(body, h.body_length, size)) break;
      BatchIndexEntry e{global_base + pos, p.metadata_size, static_cast<int32_t>(h.type), global_base + body, h.body_length, 0};
      if (h.type == MessageType::RECORD_BATCH || h.type == MessageType::DICTIONARY_BATCH)
        e.n_rows = DecodeRecordBatch(base + pos + 8, p.metadata_size).length;
      index.push_back(e);
      pos = body + h.body_length;
    }
    global_base += size;
  }
  index_built = true;
  return index;
}

}  // namespace miarrow
