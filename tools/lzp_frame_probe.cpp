// lzp_frame_probe.cpp — lzp_staged.h's frame_from_own against container.h's frame_serial / frame_parallel, no GPU and nothing of the
// library linked.  frame_from_own frames a block from chunks that were each coded under a budget of their own size; under the serial
// rule it has to say what a chunk would have returned under the smaller budget min(size[b], n - bytes so far).  Here the chunks are
// synthetic: own[b] is drawn around every boundary of that rule (the chunk's size, the room left, room - 8, 16), and the stand-in
// encoder given to frame_serial returns own[b] where it lies below room - 8 and NOT_COMPRESSIBLE otherwise — the scanner's stopping
// rule (lzp.cpp: eob = out_end - 8).  Totals, tables, offsets and raw counts must agree.  One JSON line.
//   g++ -std=c++17 -O1 -I libbsc_amd/csrc/host tools/lzp_frame_probe.cpp -o lzp_frame_probe && ./lzp_frame_probe
#include <cstdio>
#include <cstring>
#include <vector>

#include "lzp_staged.h"

using namespace bschost;
using namespace bschost::lzp;

static unsigned long long g_state = 88172645463325252ull;
static unsigned rnd(unsigned m) { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (unsigned)(g_state % m); }

int main()
{
    const int sizes[] = {256 * 1024, 300001, (4 << 20) - 1, 4 << 20, (4 << 20) + 5, (16 << 20) - 3, (16 << 20) + 5};
    std::vector<unsigned char> out((size_t)(16 << 20) + 64);
    long cases = 0, mismatch = 0, flips = 0, not_compressible = 0, raw_by_own = 0;
    for (int n : sizes) {
        const int nc = num_chunks(n);
        for (int it = 0; it < 4000; ++it) {
            int own[8], size[8];
            // own[] is drawn chunk by chunk along the serial rule's own running offset, so that its boundaries are hit
            int optr = subtable_bytes(nc);
            for (int b = 0; b < nc; ++b) {
                size[b] = chunk_size(n, nc, b);
                const int room = size[b] < n - optr ? size[b] : n - optr;
                const int d = (int)rnd(7) - 3;
                switch (rnd(6)) {
                    case 0: own[b] = LIBBSC_NOT_COMPRESSIBLE; break;
                    case 1: own[b] = size[b] - 9 + (d > 0 ? 0 : d); break;          // the largest sizes a budget of size[b] lets through
                    case 2: own[b] = room - 8 + d; break;                           // around the smaller budget's stop
                    case 3: own[b] = 41 + (int)rnd(100); break;
                    default: own[b] = 41 + (int)rnd((unsigned)size[b] / 2); break;
                }
                if (own[b] >= size[b] - 8) own[b] = LIBBSC_NOT_COMPRESSIBLE;        // (what its own budget would have said)
                if (own[b] >= 0 && own[b] < 41) own[b] = 41;
                const bool fits = own[b] >= 0 && room >= 16 && own[b] < room - 8;
                optr += fits ? own[b] : size[b];
                if (optr > n) optr = n;
            }
            for (int features = 1; features <= 3; features += 2) {
                Frame F;
                const int got = frame_from_own(n, features, own, &F);
                int want, raws = 0, off[8];
                if (features & 2) {
                    int res[8];
                    for (int b = 0; b < nc; ++b) { res[b] = own[b] < 0 ? size[b] : own[b]; raws += own[b] < 0; }
                    want = frame_parallel(out.data(), n, nc, size, res, [&](int b, unsigned char* dst) { off[b] = (int)(dst - out.data()); return 0; });
                } else {
                    want = frame_serial(out.data(), n, nc, size,
                        [&](int b, unsigned char* dst, int room) {
                            off[b] = (int)(dst - out.data());
                            const bool fits = own[b] >= 0 && room >= 16 && own[b] < room - 8;
                            if (!fits) { ++raws; flips += own[b] >= 0; raw_by_own += own[b] < 0; }
                            return fits ? own[b] : (int)LIBBSC_NOT_COMPRESSIBLE;
                        },
                        [&](int, unsigned char*) { return 0; });
                }
                ++cases;
                not_compressible += want == LIBBSC_NOT_COMPRESSIBLE;
                bool ok = got == want && F.total == want;
                if (ok && want >= 0) {
                    unsigned char tab[1 + 8 * 8];
                    ok = frame_table(F, tab) == subtable_bytes(nc) && memcmp(tab, out.data(), (size_t)subtable_bytes(nc)) == 0 && F.raw_chunks == raws;
                    for (int b = 0; b < nc && ok; ++b) ok = F.off[b] == off[b] && F.start[b] == chunk_start(n, nc, b) && F.size[b] == size[b];
                }
                if (!ok) { if (++mismatch <= 5) fprintf(stderr, "mismatch: n %d features %d got %d want %d\n", n, features, got, want); }
            }
        }
    }
    // a single chunk: budget n - 2, one byte in front
    for (int own0 : {41, 1000, (int)LIBBSC_NOT_COMPRESSIBLE}) {
        Frame F; unsigned char tab[65];
        const int got = frame_from_own(2000, 3, &own0, &F);
        ++cases;
        if (got != (own0 < 0 ? own0 : own0 + 1) || (got >= 0 && (frame_table(F, tab) != 1 || tab[0] != 1 || F.off[0] != 1 || F.res[0] != own0))) ++mismatch;
    }
    printf("{\"cases\": %ld, \"mismatch\": %ld, \"coded_chunks_flipped_to_raw\": %ld, \"raw_by_own\": %ld, \"not_compressible\": %ld}\n",
           cases, mismatch, flips, raw_by_own, not_compressible);
    return mismatch ? 1 : 0;
}
