// book_plan_check.hip -- checks csrc/mc_launch_shape.hpp's book_plan (the chunks of a vanilla book) on the host; tests/test_book_plan.py
// builds and runs it.  Host code only; nothing is launched.  Prints one line per failed check and "all book_plan checks passed" at the end.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mc_launch_shape.hpp"

using namespace mc;

static int failures = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            ++failures;                                  \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
            printf(__VA_ARGS__);                         \
            printf("\n");                                \
        }                                                \
    } while (0)

struct Cut { uint64_t unit, units; uint32_t masked, index; };
static bool operator==(const Cut &a, const Cut &b) { return a.unit == b.unit && a.units == b.units && a.masked == b.masked && a.index == b.index; }

static std::vector<Cut> cuts_of(const BookPlan &p, int e)
{
    std::vector<Cut> v;
    const BookSpan &s = p.spans[e];
    for (uint32_t i = 0; i < s.chunks; ++i) {
        const BookChunk &c = p.chunks[s.chunk0 + i];
        v.push_back({((uint64_t)c.unit_hi << 32) | c.unit_lo, c.n_units, c.masked, c.index});
    }
    return v;
}

// every path of every entry exactly once; whole units outside the masks; no chunk across 2^32 units; masks only at the ends;
// the ticket words: every word takes at most BOOK_SHARD_CHUNKS (shards) or the shard count (top word) arrivals
static void check_plan(const std::vector<BookRange> &r, uint32_t npb, const char *what)
{
    BookPlan p;
    const BookRefusal why = book_plan(r.data(), (int)r.size(), npb, p);
    CHECK(why == BOOK_OK, "%s: refused (%d) at entry %d", what, (int)why, p.bad_entry);
    if (why != BOOK_OK) return;
    CHECK(p.spans.size() == r.size(), "%s: spans", what);
    uint32_t next_chunk = 0;
    std::vector<char> word_used(p.counter_words, 0);
    for (size_t e = 0; e < r.size(); ++e) {
        const BookSpan &s = p.spans[e];
        CHECK(s.chunk0 == next_chunk, "%s: entry %zu: chunk base", what, e);
        next_chunk += s.chunks;
        CHECK(s.shards == (s.chunks + BOOK_SHARD_CHUNKS - 1) / BOOK_SHARD_CHUNKS, "%s: entry %zu: shards", what, e);
        // the entry's ticket words: its own, inside the buffer; a sharded entry's on 128-byte lines of their own
        const uint32_t words = s.shards + (s.shards > 1 ? 1 : 0), stride = s.shards > 1 ? TICKET_STRIDE : 1;
        CHECK(s.shards == 1 || s.counter0 % TICKET_STRIDE == 0, "%s: entry %zu: sharded words not line-aligned", what, e);
        for (uint32_t w = 0; w < words; ++w) {
            const uint64_t at = (uint64_t)s.counter0 + (uint64_t)w * stride;
            CHECK(at < p.counter_words, "%s: entry %zu: ticket word outside the buffer", what, e);
            if (at < p.counter_words) {
                CHECK(!word_used[at], "%s: entry %zu: ticket word shared", what, e);
                word_used[at] = 1;
            }
        }
        uint32_t worst = s.shards > 1 ? s.shards : 0;
        for (uint32_t sh = 0; sh < s.shards; ++sh) {
            const uint32_t n = (s.chunks - sh + s.shards - 1) / s.shards;
            worst = n > worst ? n : worst;
        }
        CHECK(worst <= BOOK_SHARD_CHUNKS, "%s: entry %zu: %u arrivals on one ticket word", what, e, worst);
        const uint64_t first = r[e].first_path, end = first + r[e].n_paths;
        uint64_t path = first;   // the next path to be covered
        const std::vector<Cut> v = cuts_of(p, (int)e);
        for (size_t i = 0; i < v.size(); ++i) {
            const Cut &c = v[i];
            CHECK(c.index == i && p.chunks[s.chunk0 + i].entry == e, "%s: entry %zu chunk %zu: index/entry", what, e, i);
            CHECK(c.units >= 1 && c.units <= (1ull << 31), "%s: entry %zu chunk %zu: %llu units", what, e, i, (unsigned long long)c.units);
            CHECK((c.unit >> 32) == ((c.unit + c.units - 1) >> 32), "%s: entry %zu chunk %zu crosses 2^32 units", what, e, i);
            if (c.masked) {
                CHECK(i == 0 || i + 1 == v.size(), "%s: entry %zu: masked chunk %zu is not at an end", what, e, i);
                CHECK(c.units == 1, "%s: entry %zu: masked chunk of %llu units", what, e, (unsigned long long)c.units);
                for (uint32_t j = 0; j < npb; ++j) {
                    const uint64_t q = c.unit * npb + j;
                    const bool in = q >= first && q < end;
                    CHECK(((c.masked >> j) & 1u) == (in ? 1u : 0u), "%s: entry %zu: mask bit %u", what, e, j);
                    if (in) {
                        CHECK(q == path, "%s: entry %zu: path %llu out of order", what, e, (unsigned long long)q);
                        ++path;
                    }
                }
                CHECK(c.masked != (1u << npb) - 1, "%s: entry %zu: a whole unit was masked", what, e);
            } else {
                CHECK(c.unit * npb == path && (c.unit + c.units) * npb <= end, "%s: entry %zu chunk %zu: not whole units in range", what, e, i);
                path = (c.unit + c.units) * npb;
            }
        }
        CHECK(path == end, "%s: entry %zu: covered up to %llu of [%llu, %llu)", what, e, (unsigned long long)path, (unsigned long long)first,
              (unsigned long long)end);
    }
    CHECK(p.chunks.size() == next_chunk, "%s: totals", what);
}

int main()
{
    std::mt19937_64 rng(12345);
    const uint64_t sizes[] = {1, 3, 4, 5, 7, 8, 9, 1000, 1023, 1024, 1025, 100000, 1000000, 12500000, 100000000};
    for (uint32_t npb : {4u, 8u}) {
        // a mixed book: all sizes, aligned and offset first paths, one entry across the 2^32-unit seam, a 1e10-path entry
        std::vector<BookRange> r;
        for (uint64_t n : sizes)
            for (uint64_t off : {0ull, 1ull, 3ull, (unsigned long long)npb + 1, 123457ull})
                r.push_back({off, n});
        const uint64_t seam = (1ull << 32) * npb;
        r.push_back({seam - 1000 * npb - 3, 5000 * npb + 7});
        r.push_back({seam - 3, 10});
        r.push_back({5, 10000000000ull});
        r.push_back({(1ull << 52) - 100, 64});
        check_plan(r, npb, npb == 4 ? "mixed f32" : "mixed f64");
        for (int t = 0; t < 200; ++t) {   // random ranges
            std::vector<BookRange> q;
            for (int i = 0; i < 20; ++i)
                q.push_back({rng() % (3ull << 34), 1 + rng() % (rng() % 2 ? 100 : 100000000)});
            check_plan(q, npb, "random");
        }
        // an entry's chunks do not depend on where it sits, on the other entries or on the book's size
        BookPlan alone, big, shuffled;
        std::vector<BookRange> one = {r[0]};
        for (size_t k = 0; k < r.size(); ++k) {
            one[0] = r[k];
            book_plan(one.data(), 1, npb, alone);
            std::vector<BookRange> b2;
            for (int i = 0; i < 4000; ++i)
                b2.push_back({(uint64_t)i * 7, 1000 + (uint64_t)i});
            b2.push_back(r[k]);
            book_plan(b2.data(), (int)b2.size(), npb, big);
            CHECK(cuts_of(alone, 0) == cuts_of(big, 4000), "entry %zu moved to index 4000: other chunks", k);
        }
        std::vector<int> perm(r.size());
        for (size_t i = 0; i < perm.size(); ++i) perm[i] = (int)i;
        std::shuffle(perm.begin(), perm.end(), rng);
        std::vector<BookRange> rs;
        for (int i : perm) rs.push_back(r[i]);
        BookPlan orig;
        book_plan(r.data(), (int)r.size(), npb, orig);
        book_plan(rs.data(), (int)rs.size(), npb, shuffled);
        for (size_t i = 0; i < perm.size(); ++i)
            CHECK(cuts_of(shuffled, (int)i) == cuts_of(orig, perm[i]), "shuffled book: entry %d has other chunks", perm[i]);
        // a 1e10-path entry: bounded chunk count and arrivals on any one ticket word (checked in check_plan), a few thousand chunks at most
        std::vector<BookRange> huge = {{0, 10000000000ull}};
        BookPlan h;
        CHECK(book_plan(huge.data(), 1, npb, h) == BOOK_OK && h.spans[0].chunks <= BOOK_CHUNKS_MAX + 16, "1e10 paths: %u chunks",
              h.spans[0].chunks);
        // the refusals, with the index of the first bad entry
        const std::vector<std::pair<BookRange, BookRefusal>> bad = {
            {{0, 0}, BOOK_EMPTY},
            {{~0ull - 5, 10}, BOOK_OVERFLOW},
            {{0, (1ull << 52) + 1}, BOOK_TOO_MANY_PATHS},
            {{0, (9ull << 31) * npb}, BOOK_TOO_MANY_SEGMENTS},
        };
        for (const auto &b : bad) {
            std::vector<BookRange> q = {{0, 100}, {7, 1000}, b.first, {0, 0}};
            BookPlan p;
            const BookRefusal why = book_plan(q.data(), (int)q.size(), npb, p);
            CHECK(why == b.second && p.bad_entry == 2, "refusal %d: got %d at entry %d", (int)b.second, (int)why, p.bad_entry);
        }
        std::vector<BookRange> q = {{0, (8ull << 31) * npb}};   // the largest single call: 8 segments of 2^31 units
        BookPlan p;
        CHECK(book_plan(q.data(), 1, npb, p) == BOOK_OK, "8 segments refused");
        CHECK(BOOK_MAX_CHUNKS < (1ull << 32), "limits");
        // the book-wide chunk limit: entries of BOOK_CHUNKS_MAX chunks each, the (2^24 / 2048 + 1)-th passes it; refused with its index
        // and nothing stored (the count is known before a chunk is)
        std::vector<BookRange> many((size_t)(BOOK_MAX_CHUNKS / BOOK_CHUNKS_MAX) + 3, BookRange{0, (uint64_t)BOOK_CHUNKS_MAX * book_chunk_min(npb) * npb});
        BookPlan lim;
        std::vector<BookRange> one_big = {many[0]};
        CHECK(book_plan(one_big.data(), 1, npb, lim) == BOOK_OK && lim.spans[0].chunks == BOOK_CHUNKS_MAX, "a full entry: %u chunks",
              lim.spans[0].chunks);
        const BookRefusal why = book_plan(many.data(), (int)many.size(), npb, lim);
        CHECK(why == BOOK_TOO_MANY_CHUNKS && lim.bad_entry == (int)(BOOK_MAX_CHUNKS / BOOK_CHUNKS_MAX) && lim.chunks.empty(),
              "chunk limit: %d at entry %d, %zu chunks stored", (int)why, lim.bad_entry, lim.chunks.size());
        many.resize((size_t)(BOOK_MAX_CHUNKS / BOOK_CHUNKS_MAX) / 64);   // well inside the limit: planned
        CHECK(book_plan(many.data(), (int)many.size(), npb, lim) == BOOK_OK, "a large book refused");
    }
    if (failures == 0)
        printf("all book_plan checks passed\n");
    return failures ? 1 : 0;
}
