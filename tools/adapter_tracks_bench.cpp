// adapter_tracks_bench.cpp -- times the compiled track loop a C-ABI user has today: include/lvba_adapter.hpp's
// build_tracks_and_fuse_with (match graph, BFS components, the two size checks, the packing of every order with its uv) with a
// fusion that accepts every component, on a match set written by tools/tracks_bench.py.  The competitor of lvba_trackgraph_create
// + lvba_trackgraph_orders.  CPU only; links nothing of the library.
//   g++ -O2 -std=c++17 tools/adapter_tracks_bench.cpp -o tools/adapter_tracks_bench
//   tools/adapter_tracks_bench INPUT      prints {"ms": best of `repeat`, "tracks", "observations", "checksum"}
// INPUT: int64 M, n_pairs, repeat; int64 n_keypoints [M]; int64 pairs [n_pairs][2] (i < j); int64 match_off [n_pairs + 1];
//        int32 matches [.][2]; float32 keypoints [.][2].  The match table is put into the reference's pairIndex form before the clock
//        starts: that is how the caller holds it.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>
#include "../include/lvba_adapter.hpp"

namespace {
struct KP { float x, y; };
struct TrackT {
    double Xw_fused[3];
    std::vector<std::pair<int, int>> observations;
    std::vector<int> inlier_indices;
};
struct AcceptAll {
    const std::vector<std::vector<KP>> &kps;
    lvba::FusedBatch operator()(const std::vector<std::vector<std::pair<int, int>>> &comps) const
    {
        lvba::FusedBatch out;
        std::vector<int32_t> img;
        std::vector<float> uv;
        lvba::pack_components(comps, kps, out.off, img, uv); // what lvba_fuse_tracks is handed
        out.status.assign(comps.size() + 1, 1);
        out.kept.assign(img.size() + 1, 1);
        out.X.assign(3 * (comps.size() + 1), 0.0);
        return out;
    }
};
template <class T> bool read_many(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    std::vector<int64_t> head, nk, pairs, match_off;
    std::vector<int32_t> matches;
    std::vector<float> xy;
    if (!read_many(f, head, 3)) return 1;
    const int64_t M = head[0], n_pairs = head[1], repeat = head[2];
    if (!read_many(f, nk, (size_t)M) || !read_many(f, pairs, 2 * (size_t)n_pairs) || !read_many(f, match_off, (size_t)n_pairs + 1)) return 1;
    int64_t total = 0;
    for (int64_t n : nk) total += n;
    if (!read_many(f, matches, 2 * (size_t)match_off[(size_t)n_pairs]) || !read_many(f, xy, 2 * (size_t)total)) return 1;
    fclose(f);
    std::vector<std::vector<KP>> kps((size_t)M);
    size_t k = 0;
    for (int64_t i = 0; i < M; ++i) {
        kps[(size_t)i].resize((size_t)nk[(size_t)i]);
        for (auto &p : kps[(size_t)i]) { p = KP{xy[2 * k], xy[2 * k + 1]}; ++k; }
    }
    std::vector<std::vector<std::pair<int, int>>> table((size_t)(M * (M - 1) / 2));
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int64_t i = pairs[2 * (size_t)q], j = pairs[2 * (size_t)q + 1];
        auto &m = table[(size_t)(i * (2 * M - i - 1) / 2 + (j - i - 1))];
        for (int64_t e = match_off[(size_t)q]; e < match_off[(size_t)q + 1]; ++e) m.emplace_back(matches[2 * (size_t)e], matches[2 * (size_t)e + 1]);
    }
    const AcceptAll fuse{kps};
    double best = 1e300;
    size_t n_tracks = 0, n_obs = 0;
    uint64_t checksum = 0;
    for (int64_t r = 0; r < repeat; ++r) {
        std::vector<TrackT> tracks;
        const auto t0 = std::chrono::steady_clock::now();
        lvba::build_tracks_and_fuse_with<TrackT>(kps, table, 3, fuse, tracks);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best) best = ms;
        n_tracks = tracks.size(); n_obs = 0; checksum = 0;
        for (const TrackT &t : tracks)
            for (const auto &o : t.observations) { ++n_obs; checksum += (uint64_t)o.first * 1000003u + (uint64_t)o.second; }
    }
    printf("{\"ms\": %.3f, \"tracks\": %zu, \"observations\": %zu, \"checksum\": %llu}\n", best, n_tracks, n_obs,
           (unsigned long long)(checksum % (((uint64_t)1 << 61) - 1)));
    return 0;
}
