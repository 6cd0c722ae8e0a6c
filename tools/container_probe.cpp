// container_probe.cpp — the block format of libbsc_amd/csrc/host/container.h driven from stdin; tests/test_container_host.py compares
// what it prints with the restatement in tests/pipeline_model.py, with bsc_block_info / bsc_decompress of the built library and with
// a hand-written table of the edges.  No GPU, no HIP, nothing of the library linked (the Adler-32 below is the definition):
//   g++ -std=c++17 -I libbsc_amd/csrc/host tools/container_probe.cpp -o container_probe
// One command per line, numbers separated by blanks, bytes as hex ("-": none); one JSON object per line on stdout:
//   H block_size data_size mode index adler_data adler_body       write a header, read it back, unpack and re-pack its mode
//   R <header>                                                    read a header
//   S <data>                                                      a stored block around the data
//   C n_orig mode index adler_data coded num idx[num] <payload>   a coded block around the payload (coded: its size or a negative code)
//   D <block>                                                     the decoder's view of a coded block
//   A n                                                           aux_rate
//   P n nb size[nb] res[nb]                                       the parallel framer; sub-block b is res[b] bytes of 0xC0 + b, raw 0xA0 + b
//   Q n nb size[nb] c[nb]                                         the serial framer; the stand-in coder needs c[b] bytes: with room for
//                                                                 them and c[b] < size[b] it writes them, else LIBBSC_NOT_COMPRESSIBLE
//   V n nb size[nb] res[nb]                                       serial_verdict
//   T in_size max_out <payload>                                   the table parser over the first in_size bytes
#include "container.h"
#include <cstdio>
#include <string>
#include <vector>

extern "C" unsigned int bsc_adler32(const unsigned char* T, int n, int)
{
    unsigned s1 = 1, s2 = 0;
    for (int i = 0; i < n; ++i) { s1 = (s1 + T[i]) % 65521u; s2 = (s2 + s1) % 65521u; }
    return s1 | (s2 << 16);
}

static bool read_hex(std::vector<unsigned char>& v)
{
    char buf[1 << 16];
    if (scanf("%65535s", buf) != 1) return false;
    const std::string s(buf);
    v.clear();
    if (s == "-") return true;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((unsigned char)std::stoi(s.substr(i, 2), nullptr, 16));
    return true;
}
static void print_hex(const char* name, const unsigned char* p, long long n)
{
    printf("\"%s\":\"", name);
    for (long long i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\"");
}
static bool read_ints(int* v, int n)
{
    for (int i = 0; i < n; ++i) if (scanf("%d", &v[i]) != 1) return false;
    return true;
}
static void print_fields(const BlockFields& h, bool ok)
{
    const BlockMode m = block_mode_unpack(h.mode);
    printf("\"ok\":%d,\"fields\":[%d,%d,%d,%d,%u,%u],\"mode\":[%d,%d,%d,%d],\"repacked\":%d,\"lzp\":%d", ok, h.block_size, h.data_size, h.mode, h.index,
           h.adler_data, h.adler_body, m.sorter, m.coder, m.lzp_hash, m.lzp_min, block_mode_pack(m), block_mode_has_lzp(h.mode));
}

int main()
{
    char cmd;
    std::vector<unsigned char> in;
    while (scanf(" %c", &cmd) == 1) {
        printf("{");
        if (cmd == 'H') {
            BlockFields h, back;
            if (scanf("%d %d %d %d %u %u", &h.block_size, &h.data_size, &h.mode, &h.index, &h.adler_data, &h.adler_body) != 6) return 1;
            unsigned char out[LIBBSC_HEADER_SIZE];
            block_header_write(out, h);
            const bool ok = block_header_read(out, &back);
            print_hex("bytes", out, LIBBSC_HEADER_SIZE); printf(",");
            print_fields(back, ok);
        } else if (cmd == 'R') {
            if (!read_hex(in) || in.size() < LIBBSC_HEADER_SIZE) return 1;
            BlockFields h;
            const bool ok = block_header_read(in.data(), &h);
            print_fields(h, ok);
        } else if (cmd == 'S') {
            if (!read_hex(in)) return 1;
            std::vector<unsigned char> out(in.size() + LIBBSC_HEADER_SIZE);
            if (!in.empty()) memcpy(block_body(out.data()), in.data(), in.size());
            const int r = block_finish_stored(out.data(), (int)in.size(), bsc_adler32(in.data(), (int)in.size(), 0));
            printf("\"result\":%d,", r); print_hex("bytes", out.data(), r);
        } else if (cmd == 'C') {
            int n_orig, mode, index, coded, num, idx[256]; unsigned adler;
            if (scanf("%d %d %d %u %d %d", &n_orig, &mode, &index, &adler, &coded, &num) != 6 || num < 0 || num > 255 || !read_ints(idx, num) || !read_hex(in)) return 1;
            std::vector<unsigned char> out(in.size() + LIBBSC_HEADER_SIZE + 1 + 4 * (size_t)num);
            if (!in.empty()) memcpy(block_body(out.data()), in.data(), in.size());
            const int r = block_finish_coded(out.data(), n_orig, coded, mode, index, idx, num, adler);
            printf("\"result\":%d,", r); print_hex("bytes", out.data(), r < 0 ? 0 : r);
        } else if (cmd == 'D') {
            if (!read_hex(in) || in.size() < LIBBSC_HEADER_SIZE) return 1;
            BlockFields h;
            const bool ok = block_header_read(in.data(), &h);
            CodedPayload p = {};
            const int r = ok && h.block_size >= LIBBSC_HEADER_SIZE && (size_t)h.block_size <= in.size() ? block_coded_payload(in.data(), h, &p) : 1;
            printf("\"ok\":%d,\"result\":%d,\"body_ok\":%d", ok, r, r <= 0 && block_body_ok(in.data(), h));
            if (r == LIBBSC_NO_ERROR) printf(",\"num\":%d,\"size\":%lld,\"data\":%lld,\"indexes\":%lld", p.num_indexes, p.size, (long long)(p.data - in.data()), (long long)(p.indexes - in.data()));
        } else if (cmd == 'A') {
            int n;
            if (scanf("%d", &n) != 1) return 1;
            printf("\"rate\":%d", aux_rate(n));
        } else if (cmd == 'P' || cmd == 'Q' || cmd == 'V') {
            int n, nb, size[SUBTABLE_MAX], res[SUBTABLE_MAX];
            if (scanf("%d %d", &n, &nb) != 2 || nb < 1 || nb > SUBTABLE_MAX || !read_ints(size, nb) || !read_ints(res, nb)) return 1;
            long long cap = subtable_bytes(nb);                     // what a framer may touch: table, every sub-block at its largest
            for (int b = 0; b < nb; ++b) cap += size[b];
            std::vector<unsigned char> out((size_t)cap);
            if (cmd == 'V') {
                static const char* const NAME[] = {"exact", "not_exact", "incompressible"};
                printf("\"verdict\":\"%s\"", NAME[serial_verdict(n, nb, size, res)]);
            } else if (cmd == 'P') {
                const int r = frame_parallel(out.data(), n, nb, size, res, [&](int b, unsigned char* dst) {
                    memset(dst, (res[b] != size[b] ? 0xC0 : 0xA0) + b, (size_t)res[b]);
                    return 0;
                });
                printf("\"result\":%d,", r); print_hex("bytes", out.data(), r < 0 ? 0 : r);
            } else {
                std::vector<int> rooms;
                const int r = frame_serial(out.data(), n, nb, size,
                    [&](int b, unsigned char* dst, int room) {
                        rooms.push_back(room);
                        if (res[b] >= size[b] || res[b] > room) return (int)LIBBSC_NOT_COMPRESSIBLE;
                        memset(dst, 0xC0 + b, (size_t)res[b]);
                        return res[b];
                    },
                    [&](int b, unsigned char* dst) { memset(dst, 0xA0 + b, (size_t)size[b]); return 0; });
                printf("\"result\":%d,\"rooms\":[", r);
                for (size_t i = 0; i < rooms.size(); ++i) printf("%s%d", i ? "," : "", rooms[i]);
                printf("],"); print_hex("bytes", out.data(), r < 0 ? 0 : r);
            }
        } else if (cmd == 'T') {
            long long in_size, max_out;
            if (scanf("%lld %lld", &in_size, &max_out) != 2 || !read_hex(in) || in_size > (long long)in.size()) return 1;
            const std::vector<unsigned char> cut(in.begin(), in.begin() + (in_size < 0 ? 0 : in_size));      // (a read past in_size is a read past the allocation)
            SubTableReader t;
            const int nb = subtable_open(&t, cut.data(), in_size, max_out);
            int rc = nb < 0 ? nb : LIBBSC_NO_ERROR;
            printf("\"nb\":%d,\"subs\":[", nb);
            for (int b = 0; b < nb && nb > 1 && rc == LIBBSC_NO_ERROR; ++b) {
                SubBlock s;
                rc = subtable_next(&t, &s);
                if (rc == LIBBSC_NO_ERROR) printf("%s[%d,%d,%lld,%lld]", b ? "," : "", s.isz, s.osz, s.iptr, s.optr);
            }
            printf("],\"result\":%d", rc);
        } else return 1;
        printf("}\n");
    }
    return 0;
}
