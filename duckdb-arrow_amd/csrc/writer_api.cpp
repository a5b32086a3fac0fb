// writer_api.cpp -- the C API of the encode direction (include/mi_arrow_ipc.h: mi_write_options_*, mi_writer_*, mi_ipc_*,
// mi_encode_schema) with its option parser.  The classes behind it: writer.hpp.
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "extension_format.hpp"
#include "writer_internal.hpp"

using namespace miarrow;

namespace miarrow {
int WrapC(const std::function<void()>& f);  // c_api.cpp
Context* ContextOf(mi_ctx* c);
}

namespace {
std::string LowerStr(std::string s) {
  for (auto& c : s) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
  return s;
}
std::string UpperStr(std::string s) {
  for (auto& c : s) c = static_cast<char>(std::toupper(static_cast<unsigned char>(c)));
  return s;
}

// DBConfig::ParseMemoryLimit-style sizes: "100", "1KB", "2 MiB", "1gb"
int64_t ParseMemory(const std::string& v) {
  char* end = nullptr;
  double num = std::strtod(v.c_str(), &end);
  if (end == v.c_str() || num < 0) throw InvalidInputException("Could not parse memory size '" + v + "'");
  std::string unit;
  for (const char* p = end; *p; p++)
    if (!std::isspace(static_cast<unsigned char>(*p))) unit += static_cast<char>(std::tolower(static_cast<unsigned char>(*p)));
  double mult = 1;
  if (unit.empty() || unit == "b" || unit == "byte" || unit == "bytes") mult = 1;
  else if (unit == "kb" || unit == "k") mult = 1000.0;
  else if (unit == "mb" || unit == "m") mult = 1000.0 * 1000;
  else if (unit == "gb" || unit == "g") mult = 1000.0 * 1000 * 1000;
  else if (unit == "tb" || unit == "t") mult = 1000.0 * 1000 * 1000 * 1000;
  else if (unit == "kib") mult = 1024.0;
  else if (unit == "mib") mult = 1024.0 * 1024;
  else if (unit == "gib") mult = 1024.0 * 1024 * 1024;
  else if (unit == "tib") mult = 1024.0 * 1024 * 1024 * 1024;
  else throw InvalidInputException("Unknown unit for memory size: '" + unit + "'");
  return static_cast<int64_t>(num * mult);
}

uint64_t ParseU64(const std::string& name, const std::string& v) {
  char* end = nullptr;
  errno = 0;
  unsigned long long x = std::strtoull(v.c_str(), &end, 10);
  if (end == v.c_str() || *end != 0 || errno != 0 || (!v.empty() && v[0] == '-'))
    throw InvalidInputException("Could not convert string '" + v + "' to UINT64 for option " + UpperStr(name));
  return x;
}

// arrow_large_buffer_size: VARCHAR / BLOB / LIST export with 64-bit offsets (ArrowConverter::ToArrowSchema with
// ArrowOffsetSize::LARGE); MAP keeps int32 offsets (the Arrow format has no large map)
void MakeLarge(ArrowField& f) {
  if (f.type == MI_AT_UTF8) f.type = MI_AT_LARGE_UTF8;
  else if (f.type == MI_AT_BINARY) f.type = MI_AT_LARGE_BINARY;
  else if (f.type == MI_AT_LIST) f.type = MI_AT_LARGE_LIST;
  for (auto& c : f.children) MakeLarge(c);
}

// produce_arrow_string_view: VARCHAR at any depth exports as Utf8View, whatever arrow_large_buffer_size says (ArrowConverter::
// ToArrowSchema asks for the view property first); BLOB is not touched (DuckDB writes no binary views)
void MakeView(ArrowField& f) {
  // (a UUID column stays utf8 / large_utf8: DuckDB's switch for UUID looks at the offset size alone)
  if (f.type == MI_AT_UTF8 && f.extension != extfmt::kUuid) f.type = MI_AT_UTF8_VIEW;
  for (auto& c : f.children) MakeView(c);
}

std::vector<ArrowField> FieldsFromC(const mi_field* fields, int32_t n_fields, bool large = false, bool views = false) {
  if (!fields || n_fields <= 0) throw InvalidInputException("writer needs at least one column");
  std::vector<ArrowField> out;
  for (int32_t i = 0; i < n_fields; i++) {
    out.push_back(FieldFromDuckType(fields[i].name, fields[i].duck_type));
    if (views) MakeView(out.back());
    if (large) MakeLarge(out.back());
  }
  return out;
}
}  // namespace

extern "C" {

int mi_write_options_init(mi_write_options* o) {
  return WrapC([&] {
    if (!o) throw InvalidInputException("mi_write_options_init: NULL");
    std::memset(o, 0, sizeof(*o));
    o->row_group_size = 122880;
    o->preserve_insertion_order = 1;
  });
}

int mi_write_options_set(mi_write_options* o, const char* name, const char* value) {
  return WrapC([&] {
    if (!o || !name) throw InvalidInputException("mi_write_options_set: NULL");
    const std::string loption = LowerStr(name);
    if (!value) throw BinderException(UpperStr(loption) + " requires exactly one argument");
    if (loption == "row_group_size" || loption == "chunk_size") {
      if (o->row_group_size_set) throw BinderException("ROW_GROUP_SIZE and ROW_GROUP_SIZE_BYTES are mutually exclusive");
      o->row_group_size = static_cast<int64_t>(ParseU64(loption, value));
      o->row_group_size_set = 1;
    } else if (loption == "row_group_size_bytes") {
      o->row_group_size_bytes = ParseMemory(value);
      o->row_group_size_bytes_set = 1;
    } else if (loption == "row_groups_per_file") {
      o->row_groups_per_file = static_cast<int64_t>(ParseU64(loption, value));
    } else if (loption == "compression" || loption == "codec") {
      const std::string codec = LowerStr(value);
      if (codec == "uncompressed" || codec == "none") o->compression = MI_WRITE_COMPRESSION_NONE;
      else if (codec == "lz4" || codec == "lz4_frame") o->compression = MI_WRITE_COMPRESSION_LZ4_FRAME;
      else if (codec == "zstd") throw NotImplementedException("COMPRESSION zstd: ZSTD bodies are read but not written by this path (use lz4 or uncompressed)");
      else throw BinderException("Unknown COMPRESSION '" + std::string(value) + "' for FORMAT ARROWS: expected uncompressed, none, lz4 or lz4_frame");
    }
    // other options are not ours: the bind loop ignores them (write_arrow_stream.cpp:62-105) -- produce_arrow_string_view and
    // arrow_large_buffer_size among them: those are settings, which reach the struct's fields from the client's properties
  });
}

int mi_write_options_add_kv(mi_write_options* o, const char* key, const char* value, int32_t value_len) {
  return WrapC([&] {
    if (!o || !key || !value) throw InvalidInputException("mi_write_options_add_kv: NULL");
    if (o->n_kv_metadata >= MI_MAX_KV_METADATA) throw InvalidInputException("too many kv_metadata entries");
    if (value_len < 0) value_len = static_cast<int32_t>(std::strlen(value));
    if (std::strlen(key) >= sizeof(o->kv_keys[0]) || static_cast<size_t>(value_len) > sizeof(o->kv_values[0]))
      throw InvalidInputException("kv_metadata entry too long");
    std::snprintf(o->kv_keys[o->n_kv_metadata], sizeof(o->kv_keys[0]), "%s", key);
    std::memcpy(o->kv_values[o->n_kv_metadata], value, static_cast<size_t>(value_len));
    o->kv_value_lens[o->n_kv_metadata] = value_len;
    o->n_kv_metadata++;
  });
}

int mi_write_options_finalize(mi_write_options* o) {
  return WrapC([&] {
    if (!o) throw InvalidInputException("mi_write_options_finalize: NULL");
    if (o->row_group_size_bytes_set) {
      if (o->preserve_insertion_order) {
        throw BinderException(
            "ROW_GROUP_SIZE_BYTES does not work while preserving insertion order. Use \"SET "
            "preserve_insertion_order=false;\" to disable preserving insertion order.");
      }
    } else {
      // We always set a max row group size bytes so we don't use too much memory
      o->row_group_size_bytes = o->row_group_size * 1024;
    }
  });
}

int mi_encode_schema(const mi_field* fields, int32_t n_fields, uint8_t* out, int64_t cap, int64_t* size) {
  return WrapC([&] {
    if (!size) throw InvalidInputException("mi_encode_schema: NULL argument");
    ArrowSchemaModel schema;
    schema.fields = FieldsFromC(fields, n_fields);
    const std::vector<uint8_t> msg = EncodeSchemaMessage(schema);
    *size = static_cast<int64_t>(msg.size());
    if (out && cap >= *size) std::memcpy(out, msg.data(), msg.size());
  });
}

int mi_writer_open(mi_ctx* ctx, const char* path, const mi_field* fields, int32_t n_fields, const mi_write_options* opts,
                   mi_writer** out) {
  return WrapC([&] {
    if (!ctx || !path || !out) throw InvalidInputException("mi_writer_open: NULL argument");
    auto w = std::make_unique<mi_writer>();
    w->ctx = ContextOf(ctx);
    if (opts) {
      w->opts = *opts;
    } else {
      mi_write_options_init(&w->opts);
      mi_write_options_finalize(&w->opts);
    }
    if (w->opts.row_group_size_bytes <= 0) w->opts.row_group_size_bytes = w->opts.row_group_size * 1024;
    w->fields = FieldsFromC(fields, n_fields, w->opts.arrow_large_buffer_size != 0, w->opts.produce_arrow_string_view != 0);
    std::vector<std::pair<std::string, std::string>> kv;
    for (int32_t i = 0; i < w->opts.n_kv_metadata; i++)
      kv.emplace_back(w->opts.kv_keys[i], std::string(w->opts.kv_values[i], static_cast<size_t>(w->opts.kv_value_lens[i])));
    w->buffer = std::make_unique<ChunkCollection>(PinnedStaging(w->ctx), w->fields);
    if (w->opts.compression != MI_WRITE_COMPRESSION_NONE && w->opts.compression != MI_WRITE_COMPRESSION_LZ4_FRAME)
      throw InvalidInputException("mi_write_options.compression " + std::to_string(w->opts.compression) + " is not a codec of this writer");
    w->writer = std::make_unique<ArrowStreamWriter>(w->ctx, path, w->fields, kv, w->opts.compression);
    w->writer->WriteSchema();
    *out = w.release();
  });
}

int mi_writer_sink(mi_writer* w, const mi_data_chunk* chunk) {
  return WrapC([&] {
    if (!w || !chunk || !w->writer) throw InvalidInputException("mi_writer_sink: bad argument");
    // append data to the local (buffered) chunk collection; flush when it exceeds the row / byte budget
    TimedAppend(*w->buffer, *chunk);
    if (w->buffer->Count() >= w->opts.row_group_size || w->buffer->SizeInBytes() >= w->opts.row_group_size_bytes) {
      w->writer->Flush(*w->buffer);
    }
  });
}

int mi_writer_local_create(mi_writer* w, mi_writer_local** out) {
  return WrapC([&] {
    if (!w || !w->writer || !out) throw InvalidInputException("mi_writer_local_create: bad argument");
    *out = MakeLocal(w).release();
  });
}

int mi_writer_local_sink(mi_writer_local* l, const mi_data_chunk* chunk) {
  return WrapC([&] {
    if (!l || !chunk) throw InvalidInputException("mi_writer_local_sink: bad argument");
    TimedAppend(*l->buffer, *chunk);
    if (l->buffer->Count() >= l->w->opts.row_group_size || l->buffer->SizeInBytes() >= l->w->opts.row_group_size_bytes) l->FlushRowGroup();
  });
}

int mi_writer_local_combine(mi_writer_local* l) {
  return WrapC([&] {
    if (!l) throw InvalidInputException("mi_writer_local_combine: NULL");
    if (l->buffer->Count() > 0) l->FlushRowGroup();
  });
}

void mi_writer_local_destroy(mi_writer_local* l) { delete l; }

int mi_writer_finalize(mi_writer* w) {
  return WrapC([&] {
    if (!w || !w->writer) throw InvalidInputException("mi_writer_finalize: bad argument");
    if (w->buffer->Count() > 0) w->writer->Flush(*w->buffer);  // ArrowWriteCombine
    w->writer->Finalize();                                     // ArrowWriteFinalize
  });
}

void mi_writer_close(mi_writer* w) { delete w; }

int64_t mi_writer_row_groups(const mi_writer* w) { return (w && w->writer) ? static_cast<int64_t>(w->writer->NumberOfRowGroups()) : 0; }
int64_t mi_writer_file_size(const mi_writer* w) { return (w && w->writer) ? static_cast<int64_t>(w->writer->FileSize()) : 0; }

int mi_writer_rotate_next_file(const mi_writer* w, int64_t file_size_bytes) {
  if (!w || !w->writer) return 0;
  if (file_size_bytes >= 0 && static_cast<int64_t>(w->writer->FileSize()) > file_size_bytes) return 1;
  if (w->opts.row_groups_per_file > 0 && static_cast<int64_t>(w->writer->NumberOfRowGroups()) >= w->opts.row_groups_per_file) return 1;
  return 0;
}

int mi_ipc_serializer_create(mi_ctx* ctx, const mi_field* fields, int32_t n_fields, mi_writer** out) {
  return WrapC([&] {
    if (!ctx || !out) throw InvalidInputException("mi_ipc_serializer_create: NULL argument");
    auto w = std::make_unique<mi_writer>();
    w->ctx = ContextOf(ctx);
    mi_write_options_init(&w->opts);
    w->fields = FieldsFromC(fields, n_fields);
    w->schema.fields = w->fields;
    w->buffer = std::make_unique<ChunkCollection>(PinnedStaging(w->ctx), w->fields);
    w->serializer = std::make_unique<ColumnDataCollectionSerializer>(w->ctx);
    w->serializer->Init(&w->schema);
    *out = w.release();
  });
}

int mi_ipc_serialize_schema(mi_writer* w, const uint8_t** blob, int64_t* size) {
  return WrapC([&] {
    if (!w || !w->serializer || !blob || !size) throw InvalidInputException("mi_ipc_serialize_schema: bad argument");
    w->serializer->SerializeSchema();
    w->blob = w->serializer->GetHeader();
    *blob = w->blob.data();
    *size = static_cast<int64_t>(w->blob.size());
  });
}

int mi_writer_append_message(mi_writer* w, const uint8_t* blob, int64_t size) {
  return WrapC([&] {
    if (!w || !w->writer || (!blob && size) || size < 0) throw InvalidInputException("mi_writer_append_message: bad argument");
    if (size == 0) {   // an empty collection still counts as a flushed row group (ArrowStreamWriter::Flush)
      w->writer->CountEmptyFlush();
      return;
    }
    w->writer->WriteMessage(blob, static_cast<size_t>(size), nullptr, 0);
  });
}

int mi_ipc_serialize_chunks(mi_writer* w, const mi_data_chunk* chunks, int32_t n_chunks, const uint8_t** blob, int64_t* size) {
  return WrapC([&] {
    if (!w || !w->serializer || !blob || !size || (!chunks && n_chunks)) throw InvalidInputException("mi_ipc_serialize_chunks: bad argument");
    w->buffer->Reset();
    for (int32_t i = 0; i < n_chunks; i++) TimedAppend(*w->buffer, chunks[i]);
    w->blob.clear();
    if (w->serializer->Serialize(*w->buffer)) {
      // header || body concatenated, like SerializeArray (to_arrow_ipc.cpp:72-87)
      const auto& h = w->serializer->GetHeader();
      w->blob.resize(h.size() + static_cast<size_t>(w->serializer->GetBodySize()));
      std::memcpy(w->blob.data(), h.data(), h.size());
      std::memcpy(w->blob.data() + h.size(), w->serializer->GetBody(), static_cast<size_t>(w->serializer->GetBodySize()));
    }
    w->buffer->Reset();
    *blob = w->blob.data();
    *size = static_cast<int64_t>(w->blob.size());
  });
}

}  // extern "C"
