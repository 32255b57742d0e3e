// capi_tile_masks.hip -- the tile mask table behind the C boundary (kernels_tile_masks.hip; DESIGN.md section 3, "The tile mask
// table"): how a call builds it -- over this rank's keyframes and two sums over the ranks under keyframe sharding, over all keyframes
// and without an exchange on route 1 -- and the three entry points of the observed structure computed from it
// (bahip_observed_covisibility, bahip_keyframe_observer_histogram, bahip_surfel_observations hand over after their refusals).
// The sequence of exchanges of a call depends on replicated values only: the tiles, the world, the entries E, the pairs P, the
// caller's capacity and planes and the slice settings.  The table is rebuilt by every call.
#include <algorithm>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
constexpr int kStageCount = 1, kStageFill = 2, kStageMerge = 4, kStageConsumer = 8, kStageAll = 15;
// a slice of either exchange is about 16 MB, like the rows of the per-surfel cost: 10 bytes per entry, 4 per payload word
constexpr uint32_t kDefaultEntrySlice = 1600000u, kDefaultPayloadSlice = 4000000u;
enum { kCounterListed = 0, kCounterAdds = 1, kCounterPayload = 2, kCounterPairs = 3, kCounters = 4 };

TileMaskShape g_shape{kTileMaskDefaultWaves, 0};   // workgroups 0: kTileMaskWorkgroupsPerUnit per compute unit
int g_tile_order = 1;
uint32_t g_entry_slice = kDefaultEntrySlice, g_payload_slice = kDefaultPayloadSlice;
int g_route = 0;
int g_stages = kStageAll;   // what a call launches (scripts/observed_structure_table_eval.py times the stages by difference)

int default_workgroups() {
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return kTileMaskWorkgroupsPerUnit * units;
}
TileMaskShape launch_shape() { return TileMaskShape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups()}; }

int exchange_failed(const char* what) {
  return fail((std::string("the sum of the ") + what + " over the ranks failed (" + g_last_error + ")").c_str(), __FILE__, __LINE__);
}

// The partition a call works under: the keyframe partition under keyframe sharding (the traversals filter by owner, the table is
// exchanged, the tiles of the reductions are dealt), none on route 1 elsewhere.
struct Partition {
  bool sharded;
  uint32_t rank, world;
};
Partition partition_of(const bahip_context* ctx) {
  if (kf_sharded(ctx)) return Partition{true, (uint32_t)ctx->kf_rank, (uint32_t)ctx->kf_world};
  return Partition{false, 0u, 1u};
}

// The table of the surfels of `v` (at least one) over the bound keyframes (at least one, fewer than 65 536) into the context's planes.
int build_table(bahip_context* ctx, const SurfelsView& v, const Partition& part, TileMaskTable* table) {
  const int K = ctx->num_kfs;
  const uint32_t T = surfel_tiles(v.size);
  const uint32_t plane_words = (part.world + 3u) / 4u;
  const size_t tile_words = (size_t)T + 1;
  ctx->tile_mask_valid = false;
  ctx->tile_mask_exchanges = 0;
  ctx->tile_mask_consumer_tiles = 0;
  REQUIRE(tile_words <= (size_t)0x7fffffff, "the tile mask table: too many tiles for the scan");
  if (ctx->tile_mask_words.reserve(4 * tile_words, tile_words / 2, "the per-tile words of the tile mask table")) return 1;
  if (ctx->tile_mask_plane.reserve((size_t)T * plane_words, (size_t)T * plane_words / 8, "the count plane of the tile mask table")) return 1;
  if (ctx->tile_mask_counters.reserve(kCounters, 0, "the counters of the tile mask table")) return 1;
  if (ctx->tile_mask_scan_temp.reserve(scan_temp_bytes(tile_words), 0, "the scan of the tile mask table")) return 1;
  uint32_t* counts = ctx->tile_mask_words;
  uint32_t* totals = counts + tile_words;
  uint32_t* rank_offset = totals + tile_words;
  uint32_t* tile_first = rank_offset + tile_words;
  Intrinsics in = ctx->in;
  in.fast_math = 0;   // (read by dispatchers only; this unit has one flavour)
  const uint32_t* sched = g_tile_order ? tile_order_for(ctx, v.size) : nullptr;
  const TileMaskShape shape = launch_shape();
  const uint32_t owner_mask = part.world - 1u;
  HIP_TRY(hipMemsetAsync(ctx->tile_mask_counters, 0, kCounters * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(hipMemsetAsync(counts, 0, tile_words * sizeof(uint32_t), ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->tile_mask_plane, 0, (size_t)T * plane_words * sizeof(long long), ctx->stream));
  if (g_stages & kStageCount) {
    launch_tile_mask_count(ctx->stream, in, ctx->dev_kfs, K, owner_mask, part.rank, v, sched, shape, counts, ctx->tile_mask_plane, plane_words,
                           ctx->tile_mask_counters + kCounterListed);
    CHECK_LAUNCH();
  }
  if (part.sharded) {
    ++ctx->tile_mask_exchanges;
    if (reduce_over_ranks(ctx, ctx->tile_mask_plane, (size_t)T * plane_words, BAHIP_SUM_I64)) return exchange_failed("tile mask counts");
  }
  launch_tile_mask_offsets(ctx->stream, ctx->tile_mask_plane, plane_words, T, part.rank, part.world, totals, rank_offset);
  CHECK_LAUNCH();
  HIP_TRY(scan_u32_exclusive(ctx->stream, ctx->tile_mask_scan_temp, ctx->tile_mask_scan_temp.size(), totals, tile_first, (int)tile_words));
  uint32_t E = 0;
  HIP_TRY(hipMemcpyAsync(&E, tile_first + T, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));   // the one host wait of the table
  const size_t room = std::max<size_t>(E, 1);
  if (ctx->tile_mask_raw_keyframes.reserve(room, room / 8, "the entries of the tile mask table")) return 1;
  if (ctx->tile_mask_raw_masks.reserve(room, room / 8, "the entries of the tile mask table")) return 1;
  if (ctx->tile_mask_keyframes.reserve(room, room / 8, "the entries of the tile mask table")) return 1;
  if (ctx->tile_mask_masks.reserve(room, room / 8, "the entries of the tile mask table")) return 1;
  if (E > 0) {
    HIP_TRY(hipMemsetAsync(ctx->tile_mask_raw_keyframes, 0, (size_t)E * sizeof(uint32_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->tile_mask_raw_masks, 0, (size_t)E * sizeof(unsigned long long), ctx->stream));
    if (g_stages & kStageFill) {
      launch_tile_mask_fill(ctx->stream, in, ctx->dev_kfs, K, owner_mask, part.rank, v, sched, shape, counts, tile_first, rank_offset, E,
                            ctx->tile_mask_raw_keyframes, ctx->tile_mask_raw_masks);
      CHECK_LAUNCH();
    }
    if (part.sharded) {
      const uint32_t slice = std::min(E, g_entry_slice);
      if (ctx->tile_mask_stage.reserve(tile_mask_slice_words(slice), 0, "a slice of the tile mask entries")) return 1;
      for (uint32_t begin = 0; begin < E; begin += slice) {
        const uint32_t count = std::min(slice, E - begin);
        launch_tile_mask_pack(ctx->stream, ctx->tile_mask_raw_keyframes, ctx->tile_mask_raw_masks, begin, count, ctx->tile_mask_stage);
        CHECK_LAUNCH();
        ++ctx->tile_mask_exchanges;
        if (reduce_over_ranks(ctx, ctx->tile_mask_stage, tile_mask_slice_words(count), BAHIP_SUM_I64)) return exchange_failed("tile mask entries");
        launch_tile_mask_unpack(ctx->stream, ctx->tile_mask_stage, begin, count, ctx->tile_mask_raw_keyframes, ctx->tile_mask_raw_masks);
        CHECK_LAUNCH();
      }
    }
    if (g_stages & kStageMerge) {
      launch_tile_mask_merge(ctx->stream, shape, tile_first, T, E, ctx->tile_mask_raw_keyframes, ctx->tile_mask_raw_masks, ctx->tile_mask_keyframes,
                             ctx->tile_mask_masks);
      CHECK_LAUNCH();
    }
  }
  ctx->tile_mask_tiles = T;
  ctx->tile_mask_entries = E;
  ctx->tile_mask_valid = g_stages == kStageAll;
  *table = TileMaskTable{tile_first, ctx->tile_mask_keyframes, ctx->tile_mask_masks, T, E};
  return 0;
}

uint32_t dealt_tiles(uint32_t tiles, const Partition& part) { return tiles > part.rank ? (tiles - part.rank + part.world - 1u) / part.world : 0u; }

// A plane of 32-bit words summed over the ranks as bit patterns, in slices of at most g_payload_slice words.
int exchange_words(bahip_context* ctx, uint32_t* plane, size_t words) {
  const size_t slice = std::min<size_t>(words, g_payload_slice);
  if (ctx->tile_mask_stage.reserve((slice + 1) / 2, 0, "a slice of the observation payload")) return 1;
  for (size_t begin = 0; begin < words; begin += slice) {
    const uint32_t count = (uint32_t)std::min(slice, words - begin);
    launch_tile_mask_words_pack(ctx->stream, plane, begin, count, ctx->tile_mask_stage);
    CHECK_LAUNCH();
    ++ctx->tile_mask_exchanges;
    if (reduce_over_ranks(ctx, ctx->tile_mask_stage, (count + 1u) / 2u, BAHIP_SUM_I64)) return exchange_failed("observation payload");
    launch_tile_mask_words_unpack(ctx->stream, ctx->tile_mask_stage, begin, count, plane);
    CHECK_LAUNCH();
  }
  return 0;
}
}  // namespace

namespace bahip_capi {

bool observed_structure_by_table(const bahip_context* ctx) { return kf_sharded(ctx) || g_route == 1; }

int tile_mask_covisibility(bahip_context* ctx, const bahip_surfels* surfels, uint32_t* counts, int pitch_words) {
  const int K = ctx->num_kfs;
  const SurfelsView v = make_view(surfels);
  const Partition part = partition_of(ctx);
  if (ctx->covis_census.reserve(3, 0, "the co-visibility census")) return 1;
  if (part.sharded && v.size == 0) {   // (replicated: every rank returns here, before any exchange)
    HIP_TRY(hipMemsetAsync(ctx->covis_census, 0, 3 * sizeof(unsigned long long), ctx->stream));
    launch_covisibility_clear(ctx->stream, counts, K, (uint32_t)pitch_words);
    CHECK_LAUNCH();
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
  }
  const bool exchange = is_sharded(ctx);   // the keyframe partition's sum, or the surfel shards' (an empty shard joins it)
  const size_t words = (size_t)K * (size_t)K;
  uint32_t* rows = counts;
  uint32_t pitch = (uint32_t)pitch_words;
  long long* wide = nullptr;
  if (exchange) {
    // [words int64 | words uint32]
    if (ctx->covis_stage.reserve(words + (words + 1) / 2, 0, "the co-visibility words of a shard")) return 1;
    wide = ctx->covis_stage;
    rows = reinterpret_cast<uint32_t*>(wide + words);
    pitch = (uint32_t)K;
  }
  TileMaskTable table{nullptr, nullptr, nullptr, 0u, 0u};
  if (v.size > 0) {
    if (build_table(ctx, v, part, &table)) return 1;
  } else {
    if (ctx->tile_mask_counters.reserve(kCounters, 0, "the counters of the tile mask table")) return 1;
    HIP_TRY(hipMemsetAsync(ctx->tile_mask_counters, 0, kCounters * sizeof(unsigned long long), ctx->stream));
    ctx->tile_mask_valid = false;
    ctx->tile_mask_exchanges = 0;
    ctx->tile_mask_consumer_tiles = 0;
  }
  launch_covisibility_clear(ctx->stream, rows, K, pitch);
  CHECK_LAUNCH();
  if (g_stages & kStageConsumer) {
    launch_tile_mask_covisibility(ctx->stream, launch_shape(), table, part.rank, part.world, K, rows, pitch, ctx->tile_mask_counters + kCounterAdds);
    CHECK_LAUNCH();
    launch_covisibility_mirror(ctx->stream, rows, K, pitch);   // the reduction sums the lower triangle
    CHECK_LAUNCH();
    ctx->tile_mask_consumer_tiles = dealt_tiles(table.tiles, part);
  }
  launch_tile_mask_census(ctx->stream, table.entries, ctx->tile_mask_counters + kCounterAdds, ctx->covis_census);
  CHECK_LAUNCH();
  if (exchange) {
    launch_covisibility_widen(ctx->stream, rows, K, wide);
    CHECK_LAUNCH();
    ++ctx->tile_mask_exchanges;
    if (reduce_over_ranks(ctx, wide, words, BAHIP_SUM_I64)) return exchange_failed("co-visibility words");
    launch_covisibility_narrow(ctx->stream, wide, K, counts, (uint32_t)pitch_words);
    CHECK_LAUNCH();
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int tile_mask_histogram(bahip_context* ctx, const bahip_surfels* surfels, int bins, uint32_t* hist, int pitch_words) {
  const int K = ctx->num_kfs;
  const SurfelsView v = make_view(surfels);
  const Partition part = partition_of(ctx);
  if (ctx->redundancy_census.reserve(3, 0, "the keyframe redundancy census")) return 1;
  if (part.sharded && v.size == 0) {   // (replicated: every rank returns here, before any exchange)
    HIP_TRY(hipMemsetAsync(ctx->redundancy_census, 0, 3 * sizeof(unsigned long long), ctx->stream));
    launch_redundancy_clear(ctx->stream, hist, K, bins, (uint32_t)pitch_words);
    CHECK_LAUNCH();
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
  }
  const bool exchange = is_sharded(ctx);   // the keyframe partition's sum, or the surfel shards' (an empty shard joins it)
  const size_t words = (size_t)K * (size_t)bins;
  uint32_t* rows = hist;
  uint32_t pitch = (uint32_t)pitch_words;
  long long* wide = nullptr;
  if (exchange) {
    // [words int64 | words uint32]
    if (ctx->redundancy_stage.reserve(words + (words + 1) / 2, 0, "the keyframe redundancy words of a shard")) return 1;
    wide = ctx->redundancy_stage;
    rows = reinterpret_cast<uint32_t*>(wide + words);
    pitch = (uint32_t)bins;
  }
  TileMaskTable table{nullptr, nullptr, nullptr, 0u, 0u};
  if (v.size > 0) {
    if (build_table(ctx, v, part, &table)) return 1;
  } else {
    if (ctx->tile_mask_counters.reserve(kCounters, 0, "the counters of the tile mask table")) return 1;
    HIP_TRY(hipMemsetAsync(ctx->tile_mask_counters, 0, kCounters * sizeof(unsigned long long), ctx->stream));
    ctx->tile_mask_valid = false;
    ctx->tile_mask_exchanges = 0;
    ctx->tile_mask_consumer_tiles = 0;
  }
  launch_redundancy_clear(ctx->stream, rows, K, bins, pitch);
  CHECK_LAUNCH();
  if (g_stages & kStageConsumer) {
    launch_tile_mask_redundancy(ctx->stream, launch_shape(), table, part.rank, part.world, K, bins, rows, pitch, ctx->tile_mask_counters + kCounterAdds);
    CHECK_LAUNCH();
    ctx->tile_mask_consumer_tiles = dealt_tiles(table.tiles, part);
  }
  launch_tile_mask_census(ctx->stream, table.entries, ctx->tile_mask_counters + kCounterAdds, ctx->redundancy_census);
  CHECK_LAUNCH();
  if (exchange) {
    launch_redundancy_widen(ctx->stream, rows, (uint32_t)words, wide);
    CHECK_LAUNCH();
    ++ctx->tile_mask_exchanges;
    if (reduce_over_ranks(ctx, wide, words, BAHIP_SUM_I64)) return exchange_failed("observer histogram words");
    launch_redundancy_narrow(ctx->stream, wide, K, bins, hist, (uint32_t)pitch_words);
    CHECK_LAUNCH();
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

// (at least one keyframe and one surfel: the entry point has answered the other calls)
int tile_mask_observations(bahip_context* ctx, const bahip_surfels* surfels, const bahip_observations* out, uint64_t pair_limit, uint64_t* pairs) {
  const int K = ctx->num_kfs;
  const SurfelsView v = make_view(surfels);
  const Partition part = partition_of(ctx);
  const size_t words = (size_t)v.size + 1;
  if (ctx->obs_counts.reserve(words, words / 8, "the observation counts")) return 1;
  if (ctx->obs_scan_temp.reserve(scan_temp_bytes(words), 0, "the scan of the observation counts")) return 1;
  TileMaskTable table{nullptr, nullptr, nullptr, 0u, 0u};
  if (build_table(ctx, v, part, &table)) return 1;
  const TileMaskShape shape = launch_shape();
  uint64_t P = 0;
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the total is 64 bits");
  if (g_stages & kStageConsumer) {
    HIP_TRY(hipMemsetAsync(ctx->obs_counts + v.size, 0, sizeof(uint32_t), ctx->stream));   // the last input of the scan
    launch_tile_mask_observation_counts(ctx->stream, shape, table, v.size, ctx->obs_counts, ctx->tile_mask_counters + kCounterPairs);
    CHECK_LAUNCH();
    ctx->tile_mask_consumer_tiles = table.tiles;   // (every rank computes the lists from the whole table)
    HIP_TRY(hipMemcpyAsync(&P, ctx->tile_mask_counters + kCounterPairs, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  if (P > pair_limit) {
    char text[160];
    snprintf(text, sizeof(text), "bahip_surfel_observations: %llu pairs are more than the pair limit of %llu", (unsigned long long)P,
             (unsigned long long)pair_limit);
    return fail(text, __FILE__, __LINE__);
  }
  if (g_stages & kStageConsumer) {
    HIP_TRY(scan_u32_exclusive(ctx->stream, ctx->obs_scan_temp, ctx->obs_scan_temp.size(), ctx->obs_counts, out->surfel_first, (int)words));
    if (out->keyframes != nullptr && P <= out->capacity && P > 0) {
      launch_tile_mask_observation_keyframes(ctx->stream, shape, table, v.size, out->surfel_first, out->keyframes);
      CHECK_LAUNCH();
      if (out->depth_raw || out->descriptor_raw) {
        // the caller's planes are the zero-filled staging: a rank writes the pairs of its own keyframes, the sum is the union
        if (out->depth_raw) HIP_TRY(hipMemsetAsync(out->depth_raw, 0, (size_t)P * sizeof(float), ctx->stream));
        if (out->descriptor_raw) HIP_TRY(hipMemsetAsync(out->descriptor_raw, 0, (size_t)P * 2 * sizeof(float), ctx->stream));
        Intrinsics in = ctx->in;
        in.fast_math = 0;
        const uint32_t* sched = g_tile_order ? tile_order_for(ctx, v.size) : nullptr;
        launch_tile_mask_payload(ctx->stream, in, ctx->dev_kfs, K, part.world - 1u, part.rank, v, sched, shape, table, out->surfel_first, out->depth_raw,
                                 out->descriptor_raw, ctx->tile_mask_counters + kCounterPayload);
        CHECK_LAUNCH();
        if (part.sharded) {
          if (out->depth_raw && exchange_words(ctx, reinterpret_cast<uint32_t*>(out->depth_raw), (size_t)P)) return 1;
          if (out->descriptor_raw && exchange_words(ctx, reinterpret_cast<uint32_t*>(out->descriptor_raw), (size_t)P * 2)) return 1;
        }
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *pairs = P;
  return 0;
}

}  // namespace bahip_capi

extern "C" {
int bahip_debug_set_observed_structure_route(int route) {
  if (route != 0 && route != 1) return fail("bahip_debug_set_observed_structure_route: route 0 or 1", __FILE__, __LINE__, hipSuccess);
  g_route = route;
  return 0;
}

int bahip_debug_set_tile_mask_shape(int waves, int workgroups, int tile_order, uint32_t entry_slice, uint32_t payload_slice) {
  if (waves < 0 || waves > kTileMaskMaxWaves || workgroups < 0 || tile_order < -1 || tile_order > 1)
    return fail("bahip_debug_set_tile_mask_shape: waves 0 .. 8, workgroups >= 0, tile_order -1 .. 1", __FILE__, __LINE__, hipSuccess);
  g_shape.waves = waves ? waves : kTileMaskDefaultWaves;
  g_shape.workgroups = workgroups;
  g_tile_order = tile_order < 0 ? 1 : tile_order;
  g_entry_slice = entry_slice ? entry_slice : kDefaultEntrySlice;
  g_payload_slice = payload_slice ? payload_slice : kDefaultPayloadSlice;
  return 0;
}

int bahip_debug_set_tile_mask_stages(int stages) {
  if (stages != 0 && stages != kStageCount && stages != (kStageCount | kStageFill) && stages != (kStageCount | kStageFill | kStageMerge) &&
      stages != kStageAll)
    return fail("bahip_debug_set_tile_mask_stages: stages 0, 1, 3, 7 or 15 (every stage needs the ones before it)", __FILE__, __LINE__, hipSuccess);
  g_stages = stages ? stages : kStageAll;
  return 0;
}

int bahip_debug_read_tile_masks(bahip_context* ctx, uint32_t* tile_first, uint32_t* keyframes, uint64_t* masks, uint64_t capacity, uint64_t* entries) {
  REQUIRE(ctx != nullptr && entries != nullptr, "bahip_debug_read_tile_masks: no context or no entry count");
  REQUIRE(ctx->tile_mask_valid, "bahip_debug_read_tile_masks: the last call of this context built no table");
  const uint32_t T = ctx->tile_mask_tiles, E = ctx->tile_mask_entries;
  const uint32_t* first = ctx->tile_mask_words + 3 * ((size_t)T + 1);
  if (tile_first) HIP_TRY(hipMemcpyAsync(tile_first, first, ((size_t)T + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (E > 0 && E <= capacity) {
    if (keyframes) HIP_TRY(hipMemcpyAsync(keyframes, ctx->tile_mask_keyframes, (size_t)E * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (masks) HIP_TRY(hipMemcpyAsync(masks, ctx->tile_mask_masks, (size_t)E * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *entries = E;
  return 0;
}

int bahip_debug_tile_mask_stats(bahip_context* ctx, uint64_t out[6]) {
  REQUIRE(ctx != nullptr && out != nullptr, "bahip_debug_tile_mask_stats: no context or no output");
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (!ctx->tile_mask_counters.get()) return 0;   // no call yet
  uint64_t counters[kCounters];
  HIP_TRY(hipMemcpyAsync(counters, ctx->tile_mask_counters, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  out[0] = counters[kCounterListed];
  out[1] = ctx->tile_mask_valid ? ctx->tile_mask_entries : 0;
  out[2] = (uint64_t)ctx->tile_mask_exchanges;
  out[3] = (uint64_t)ctx->tile_mask_consumer_tiles;
  out[4] = counters[kCounterAdds];
  out[5] = counters[kCounterPayload];
  return 0;
}
}  // extern "C"
