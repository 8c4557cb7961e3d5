// The host-only half of the cohort's outputs (malva_amd/host/part_file.hpp, malva_amd/host/cohort_out.hpp) driven without a device:
// the PATH.part -> PATH hand-over and its scratch kind, the text of the --pairs and --sample-stats tables on hand-written tables, the
// site-counts and packed-calls streams written and read back (and cut short), the two paste passes over made-up blocks.  Meant to be
// built with -fsanitize=address,undefined and run on the CPU (`make sanitize-host`); tests/test_cohort_out_cpu.py builds it plain.
// It takes a scratch directory as its argument and exits non-zero on the first wrong answer.
#include <cstdio>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>

#include "cohort_out.hpp"

using namespace malva;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond "\n";       \
            std::cout << "cohort_out_host_check: FAILED\n";                    \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static bool exists(const std::string &p) { return access(p.c_str(), F_OK) == 0; }
static std::string slurp(const std::string &p)
{
    std::ifstream in(p, std::ios::binary);
    std::stringstream all;
    all << in.rdbuf();
    return all.str();
}
// the message of the std::runtime_error `run` ends in, or the empty string
static std::string error_of(const std::function<void()> &run)
{
    try {
        run();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return std::string();
}
static bool has(const std::string &text, const char *piece) { return text.find(piece) != std::string::npos; }
// scratch files with the given contents, as a panel pass leaves them: written, closed, still there
static void fill(std::deque<PartFile> &files, const std::string &base, const std::vector<std::string> &contents)
{
    for (size_t g = 0; g < contents.size(); ++g) {
        files.emplace_back();
        files.back().open(base + ".g" + std::to_string(g) + ".part", PartFile::SCRATCH);
        files.back().write(contents[g]);
        files.back().finish();
    }
}
static std::string inflate_bgzf(const std::string &bytes, std::string &last_member)
{
    std::string plain;
    for (size_t at = 0; at < bytes.size();) {
        CHECK(at + 18 <= bytes.size() && (unsigned char)bytes[at] == 0x1f && (unsigned char)bytes[at + 1] == 0x8b && bytes[at + 12] == 'B' && bytes[at + 13] == 'C');
        const size_t size = ((unsigned char)bytes[at + 16] | (size_t)(unsigned char)bytes[at + 17] << 8) + 1;
        CHECK(size >= 26 && at + size <= bytes.size());
        uint32_t isize;
        memcpy(&isize, &bytes[at + size - 4], 4);
        std::string piece((size_t)isize + 1, '\0'); // (one byte to spare: the empty member inflates into nothing)
        z_stream zs{};
        CHECK(inflateInit2(&zs, -15) == Z_OK);
        zs.next_in = (Bytef *)&bytes[at + 18];
        zs.avail_in = (uInt)(size - 26);
        zs.next_out = (Bytef *)&piece[0];
        zs.avail_out = isize + 1;
        const int rc = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        CHECK(rc == Z_STREAM_END && zs.total_out == isize);
        plain.append(piece, 0, isize);
        last_member = bytes.substr(at, size);
        at += size;
    }
    return plain;
}

static void check_part_file(const std::string &dir)
{
    const std::string path = dir + "/cohort_out_host_check.out";
    {
        PartFile f;
        f.write("ignored", 7); // (not open: nothing happens)
        f.open(path);
        CHECK(exists(path + ".part") && !exists(path));
        f.write("abc", 3);
        f.write(std::string("def"), "never thrown");
        f.finish();
        CHECK(!exists(path + ".part") && slurp(path) == "abcdef");
        f.finish(); // (a second one is harmless)
        CHECK(!exists(path + ".part") && slurp(path) == "abcdef");
    }
    CHECK(slurp(path) == "abcdef");
    unlink(path.c_str());
    {
        PartFile f;
        f.open(path);
        f.write("abc", 3);
    }
    CHECK(!exists(path + ".part") && !exists(path));
    {
        PartFile f;
        const std::string nowhere = dir + "/no/such/directory/t.out";
        CHECK(error_of([&]() { f.open(nowhere); }) == "cannot write " + nowhere);
        CHECK(!exists(nowhere) && !exists(nowhere + ".part") && !exists(dir + "/no"));
    }
    const std::string scratch = path + ".g0.part";
    {
        PartFile f;
        f.open(scratch, PartFile::SCRATCH);
        f.write("xyz", 3);
        f.finish(); // closed, not renamed: a later pass reads it under this name
        CHECK(slurp(scratch) == "xyz" && f.path == scratch);
        f.finish();
    }
    CHECK(!exists(scratch) && !exists(scratch + ".part"));
    {
        PartFile f;
        f.open(scratch, PartFile::SCRATCH);
    }
    CHECK(!exists(scratch));
    {
        std::deque<PartFile> set(2); // files of one set: all closed before any is renamed
        set[0].open(path + ".a");
        set[1].open(path + ".b");
        for (PartFile &f : set) f.close();
        CHECK(exists(path + ".a.part") && exists(path + ".b.part") && !exists(path + ".a"));
        set[0].finish();
        CHECK(exists(path + ".a") && exists(path + ".b.part")); // (the other one goes with the set: a failure in between)
    }
    CHECK(exists(path + ".a") && !exists(path + ".b.part") && !exists(path + ".b"));
    unlink((path + ".a").c_str());
    PartFile::put(path, "whole");
    CHECK(slurp(path) == "whole" && !exists(path + ".part"));
    unlink(path.c_str());
}

static void check_tables()
{
    const std::string pair_head = "#A\tB\tN\tN00\tN01\tN02\tN10\tN11\tN12\tN20\tN21\tN22\tIBS0\tIBS1\tIBS2\tKING\n";
    auto cell = [](std::vector<uint64_t> &t, size_t i, size_t j, int da, int db, uint64_t v) { t[(i * 3 + j) * 9 + (size_t)(da * 3 + db)] = v; };
    // the two tables of tests/test_pairs_cpu.py::test_pairs_text_on_a_hand_written_table
    std::vector<uint64_t> t(3 * 3 * 9, 0);
    cell(t, 0, 1, 0, 1, 1); cell(t, 0, 1, 1, 2, 2); cell(t, 0, 1, 2, 0, 1);
    cell(t, 0, 2, 0, 2, 1); cell(t, 0, 2, 1, 0, 1); cell(t, 0, 2, 1, 1, 1);
    cell(t, 1, 2, 1, 2, 1); cell(t, 1, 2, 2, 0, 1); cell(t, 1, 2, 2, 1, 1); cell(t, 1, 2, 0, 2, 1);
    CHECK(pair_table_text({"a", "b", "c"}, t.data()) == pair_head +
          "a\tb\t4\t0\t1\t0\t0\t0\t2\t1\t0\t0\t1\t3\t0\t-0.6667\n"
          "a\tc\t3\t0\t0\t1\t1\t1\t0\t0\t0\t0\t1\t1\t1\t-0.3333\n"
          "b\tc\t4\t0\t0\t1\t0\t0\t1\t1\t1\t0\t2\t2\t0\t-2.0000\n");
    t.assign(3 * 3 * 9, 0);
    cell(t, 0, 1, 0, 0, 5); cell(t, 0, 1, 2, 2, 3); cell(t, 0, 1, 0, 2, 1); // no heterozygote on either side: no denominator
    cell(t, 0, 2, 0, 0, 10); cell(t, 0, 2, 1, 1, 10);
    cell(t, 1, 2, 1, 1, 1ull << 40); cell(t, 1, 2, 0, 1, 1); cell(t, 1, 2, 2, 0, 3);
    CHECK(pair_table_text({"x", "y", "z"}, t.data()) == pair_head +
          "x\ty\t9\t5\t0\t1\t0\t0\t0\t0\t0\t3\t1\t0\t8\t.\n"
          "x\tz\t20\t10\t0\t0\t0\t10\t0\t0\t0\t0\t0\t0\t20\t0.5000\n"
          "y\tz\t1099511627780\t0\t1\t0\t0\t1099511627776\t0\t3\t0\t0\t3\t1\t1099511627776\t0.5000\n");
    const std::vector<uint64_t> one(9, 0);
    CHECK(pair_table_text({"only"}, one.data()) == pair_head);

    // the table of tests/test_sample_stats_cpu.py::test_sample_stats_text_on_a_hand_written_table
    const std::string sample_head =
        "#SAMPLE\tRECORDS\tCALLED\tMASKED\tBAD\tHOM_REF\tHET\tHOM_ALT\tHET_ALT\tTS\tTV\tINS\tDEL\tOTHER\tGQ_SUM\tCOV_SUM\tNORMAL\tOVERCOV\tSINGLE\tNOCOV"
        "\tGQ_0\tGQ_10\tGQ_20\tGQ_30\tGQ_40\tGQ_50\tGQ_60\tGQ_70\tGQ_80\tGQ_90\tCALL_RATE\tHET_HOM\tTSTV\tMEAN_GQ\tMEAN_COV\n";
    std::vector<uint64_t> s(4 * MG_SAMPLE_SLOTS, 0);
    uint64_t *a = &s[0], *b = &s[MG_SAMPLE_SLOTS], *c = &s[2 * MG_SAMPLE_SLOTS];
    a[MG_SS_RECORDS] = 10; a[MG_SS_CALLED] = 8; a[MG_SS_MASKED] = 1; a[MG_SS_BAD] = 1; a[MG_SS_HOM_REF] = 3; a[MG_SS_HET] = 2; a[MG_SS_HOM_ALT] = 3;
    a[MG_SS_HET_ALT] = 1; a[MG_SS_TS] = 4; a[MG_SS_TV] = 2; a[MG_SS_INS] = 1; a[MG_SS_DEL] = 1; a[MG_SS_OTHER] = 1; a[MG_SS_GQ_SUM] = (uint64_t)(int64_t)-20;
    a[MG_SS_COV_SUM] = (1ull << 40) + 5; a[MG_SS_ST_NORMAL] = 7; a[MG_SS_ST_OVERCOV] = 1; a[MG_SS_ST_SINGLE] = 1; a[MG_SS_ST_NOCOV] = 1;
    const uint64_t gq[10] = {2, 1, 1, 1, 1, 1, 1, 0, 0, 1};
    for (int k = 0; k < 10; ++k) a[MG_SS_GQ_0 + k] = gq[k];
    b[MG_SS_RECORDS] = 3; b[MG_SS_MASKED] = 3; b[MG_SS_GQ_0] = 3; b[MG_SS_ST_NOCOV] = 3; // nothing called: MEAN_GQ has no denominator
    c[MG_SS_RECORDS] = 4; c[MG_SS_CALLED] = 4; c[MG_SS_HOM_REF] = 2; c[MG_SS_HET] = 2; c[MG_SS_TS] = 2; c[MG_SS_GQ_SUM] = 400; c[MG_SS_COV_SUM] = 6;
    c[MG_SS_ST_NORMAL] = 4; c[MG_SS_GQ_0 + 9] = 4; // no HOM_ALT, no TV; the fourth sample: no record at all
    std::string zeros;
    for (int k = 0; k < 29; ++k) zeros += "\t0";
    CHECK(sample_table_text({"a", "b", "c", "d"}, s.data()) == sample_head +
          "a\t10\t8\t1\t1\t3\t2\t3\t1\t4\t2\t1\t1\t1\t-20\t1099511627781\t7\t1\t1\t1\t2\t1\t1\t1\t1\t1\t1\t0\t0\t1\t0.8000\t0.6667\t2.0000\t-2.5000\t109951162778.1000\n"
          "b\t3\t0\t3\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t3\t3\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0.0000\t.\t.\t.\t0.0000\n"
          "c\t4\t4\t0\t0\t2\t2\t0\t0\t2\t0\t0\t0\t0\t400\t6\t4\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t4\t1.0000\t.\t.\t100.0000\t1.5000\n"
          "d" + zeros + "\t.\t.\t.\t.\t.\n");
    CHECK(sample_table_text({}, s.data()) == sample_head);
}

static void check_site_counts(const std::string &dir)
{
    const std::string base = dir + "/cohort_out_host_check.cnt";
    const char *short_file = "counts for the merged output are short";
    // three groups, records of 1, 2 and 3 alleles: group g counts ac[a] = 10 g + a + record, ns = g + 1 + record
    std::vector<std::string> streams(3);
    for (uint32_t g = 0; g < 3; ++g)
        for (uint32_t r = 0; r < 3; ++r) {
            uint32_t ac[3];
            for (uint32_t a = 0; a <= r; ++a) ac[a] = 10 * g + a + r;
            put_site_counts(streams[g], r + 1, g + 1 + r, ac);
        }
    CHECK(streams[0].size() == 3 * 8 + 4 * 6);
    {
        std::deque<PartFile> files;
        fill(files, base, streams);
        SiteCountsReader reader(files);
        std::vector<uint32_t> ac;
        for (uint32_t r = 0; r < 3; ++r) {
            uint32_t A = 0, ns = 0;
            ac.clear();
            CHECK(reader.next(A, ns, ac) && A == r + 1 && ns == 6 + 3 * r && ac.size() == A);
            for (uint32_t a = 0; a < A; ++a) CHECK(ac[a] == 30 + 3 * (a + r));
        }
        uint32_t A, ns;
        CHECK(!reader.next(A, ns, ac));
        // the same, two records at a time, in the arrays mg_format_site_info takes
        SiteCountsReader batches(files);
        std::vector<uint32_t> b_ac, b_ns, b_vao;
        batches.next_batch(2, b_ac, b_ns, b_vao);
        CHECK(b_ns == (std::vector<uint32_t>{6, 9}) && b_vao == (std::vector<uint32_t>{0, 1, 3}) && b_ac == (std::vector<uint32_t>{30, 33, 36}));
        batches.next_batch(2, b_ac, b_ns, b_vao);
        CHECK(b_ns == (std::vector<uint32_t>{12}) && b_vao == (std::vector<uint32_t>{0, 3}) && b_ac == (std::vector<uint32_t>{36, 39, 42}));
        CHECK(has(error_of([&]() { batches.next_batch(2, b_ac, b_ns, b_vao); }), short_file)); // (asked for more records than there are)
    }
    CHECK(!exists(base + ".g0.part") && !exists(base + ".g2.part"));
    for (size_t cut = 0; cut < 3; ++cut) { // one group's file 4 bytes short
        std::vector<std::string> shorter = streams;
        shorter[cut].resize(shorter[cut].size() - 4);
        std::deque<PartFile> files;
        fill(files, base, shorter);
        SiteCountsReader reader(files);
        std::vector<uint32_t> ac;
        uint32_t A, ns;
        CHECK(reader.next(A, ns, ac) && reader.next(A, ns, ac));
        CHECK(has(error_of([&]() { reader.next(A, ns, ac); }), short_file));
    }
    {
        std::vector<std::string> other = streams; // the second group's second record has three alleles, not two
        other[1].clear();
        const uint32_t ac[3] = {1, 2, 3};
        put_site_counts(other[1], 1, 1, ac);
        put_site_counts(other[1], 3, 1, ac);
        std::deque<PartFile> files;
        fill(files, base, other);
        SiteCountsReader reader(files);
        std::vector<uint32_t> got;
        uint32_t A, ns;
        CHECK(reader.next(A, ns, got));
        CHECK(has(error_of([&]() { reader.next(A, ns, got); }), short_file));
    }
}

static void check_pack_stream(const std::string &dir)
{
    const std::string base = dir + "/cohort_out_host_check.pack";
    const char *short_file = "packed calls for the pair table are short";
    // two groups of 2 and 3 planes, per batch one stream; two batches of 5 and 70 records: W = 1 and W = 2
    const size_t planes[2] = {2, 3}, records[2] = {5, 70};
    auto words_of = [&](size_t g, size_t batch) {
        std::vector<uint64_t> w(planes[g] * 3 * ((records[batch] + 63) / 64));
        for (size_t i = 0; i < w.size(); ++i) w[i] = 0x9E3779B97F4A7C15ull * (i + 1) + 1000 * g + batch;
        return w;
    };
    std::vector<std::vector<std::string>> batches(2, std::vector<std::string>(2));
    for (size_t g = 0; g < 2; ++g)
        for (size_t b = 0; b < 2; ++b) put_pack_batch(batches[g][b], b, records[b], words_of(g, b));
    CHECK(batches[0][0].size() == 16 + 8 * 6 && batches[1][1].size() == 16 + 8 * 18);
    auto walk = [&](const std::string &bytes_a, const std::string &bytes_b, size_t &seen) {
        std::deque<PartFile> files;
        fill(files, base, {bytes_a, bytes_b});
        seen = 0;
        walk_pack_pair(files[0].path, planes[0], files[1].path, planes[1], [&](size_t W, const uint64_t *a, const uint64_t *b) {
            CHECK(seen < 2 && W == (records[seen] + 63) / 64);
            const std::vector<uint64_t> want_a = words_of(0, seen), want_b = words_of(1, seen);
            CHECK(std::equal(want_a.begin(), want_a.end(), a) && std::equal(want_b.begin(), want_b.end(), b));
            ++seen;
        });
    };
    size_t seen = 0;
    walk(batches[0][0] + batches[0][1], batches[1][0] + batches[1][1], seen);
    CHECK(seen == 2);
    CHECK(has(error_of([&]() { walk(batches[0][0] + batches[0][1], batches[1][0], seen); }), short_file) && seen == 1);                   // B lacks the last batch
    CHECK(has(error_of([&]() { walk(batches[0][0], batches[1][0] + batches[1][1], seen); }), short_file) && seen == 1);                   // B has one more
    std::string other;
    put_pack_batch(other, 0, 6, words_of(1, 0));
    CHECK(has(error_of([&]() { walk(batches[0][0] + batches[0][1], other + batches[1][1], seen); }), short_file) && seen == 0);            // n_records disagree
    CHECK(has(error_of([&]() { walk(batches[0][0] + batches[0][1], batches[1][0] + batches[1][1].substr(0, 100), seen); }), short_file)); // B ends in its words
    CHECK(!exists(base + ".g0.part") && !exists(base + ".g1.part"));
    CHECK(has(error_of([&]() { walk_pack_pair(base + ".none", 2, base + ".none", 3, [](size_t, const uint64_t *, const uint64_t *) {}); }), "cannot read "));
}

static void check_paste_text(const std::string &dir)
{
    const std::string base = dir + "/cohort_out_host_check.text";
    // three blocks of 5 records: the first holds the header and whole lines, the others their sample columns alone
    std::vector<std::string> blocks(3);
    blocks[0] = "##fileformat=VCFv4.2\n##source=made up\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts0\ts1\ts2\ts3\n";
    std::string plain = blocks[0], tagged = blocks[0];
    const std::vector<std::string> infos{"AC=1;AN=8;AF=0.125;NS=4", "AN=0;NS=0", "AC=2,3;AN=6;AF=0.333333,0.5;NS=3", "AC=0;AN=2;AF=0;NS=1", "AC=8;AN=8;AF=1;NS=4"};
    for (int r = 0; r < 5; ++r) {
        const std::string fixed = "chr1\t" + std::to_string(100 + r) + "\t.\tA\tC\t.\tPASS\t", cols0 = "\tGT:GQ\t0/" + std::to_string(r % 2) + ":" + std::to_string(r),
                          cols1 = "\t1/1:" + std::to_string(10 + r) + "\t./.:0", cols2 = "\t0/1:" + std::to_string(20 + r);
        blocks[0] += fixed + "." + cols0 + "\n";
        blocks[1] += cols1 + "\n";
        blocks[2] += cols2 + "\n";
        plain += fixed + "." + cols0 + cols1 + cols2 + "\n";
        tagged += fixed + infos[(size_t)r] + cols0 + cols1 + cols2 + "\n";
    }
    size_t handed = 0, calls = 0;
    auto two_infos = [&](std::vector<char> &text, std::vector<uint64_t> &off) { // canned strings, two at a time: a seam inside the file
        text.clear();
        off.assign(1, 0);
        for (size_t i = 0; i < 2 && handed < infos.size(); ++i, ++handed) {
            text.insert(text.end(), infos[handed].begin(), infos[handed].end());
            off.push_back(text.size());
        }
        ++calls;
    };
    auto paste = [&](const std::vector<std::string> &contents, bool tags) {
        std::deque<PartFile> files;
        fill(files, base, contents);
        GroupFiles in;
        in.open(files);
        std::string out;
        handed = calls = 0;
        paste_text_groups(in.f, tags, two_infos, [&](const char *data, size_t n) { out.append(data, n); });
        return out;
    };
    CHECK(paste(blocks, false) == plain && calls == 0);
    CHECK(paste(blocks, true) == tagged && calls == 3 && handed == 5);
    std::vector<std::string> bad = blocks;
    bad[1] = blocks[1].substr(0, blocks[1].rfind("\t1/1:")); // the second block lacks its last line
    CHECK(has(error_of([&]() { paste(bad, false); }), "a group's block of the merged output is short"));
    bad = blocks;
    bad[0].replace(bad[0].find("PASS\t.\tGT") + 5, 1, "X=1"); // a record of the first block whose INFO is not '.'
    CHECK(has(error_of([&]() { paste(bad, true); }), "first block has no INFO column"));
    CHECK(paste(bad, false).find("PASS\tX=1\tGT:GQ") != std::string::npos); // (without tags nobody looks)
    CHECK(!exists(base + ".g0.part"));
}

static void check_paste_bcf(const std::string &dir)
{
    const std::string base = dir + "/cohort_out_host_check.bcf";
    // two groups of 2 and 1 samples, two records, two fields: GT (key 1, two values a sample) and GQ (key 2: int8 in the first group,
    // int16 in the second, so the paste widens); the shared block: 24 bytes of fixed fields, then what follows them
    const std::vector<uint32_t> planes{2, 1};
    const uint32_t n_fmt = 2, n_samples = 3;
    auto row = [&](size_t g, int r) {
        std::string out;
        bcf_put_typed_int(out, 1);
        bcf_put_desc(out, 2, 1);
        for (uint32_t i = 0; i < 2 * planes[g]; ++i) bcf_put_int(out, (int32_t)(2 + 2 * ((i + (uint32_t)r) % 2)), 1);
        bcf_put_typed_int(out, 2);
        bcf_put_desc(out, 1, g ? 2 : 1);
        for (uint32_t i = 0; i < planes[g]; ++i) bcf_put_int(out, g ? 300 + r : 40 + (int32_t)i + r, g ? 2 : 1);
        return out;
    };
    auto shared = [&](int r) {
        std::string out;
        for (uint32_t v : {0u, 99u + (uint32_t)r, 1u, 0x7F800001u, 2u << 16, n_fmt << 24}) bcf_put_u32(out, v); // (n_sample 0: the paste puts it right)
        bcf_put_typed_str(out, "", 0);
        bcf_put_typed_str(out, "A", 1);
        bcf_put_typed_str(out, r ? "CT" : "G", r ? 2 : 1);
        out += (char)0x11;
        out += (char)0;
        return out;
    };
    BcfHeader hdr;
    hdr.ids = {{"PASS", 0}, {"AC", 3}, {"AN", 4}, {"AF", 5}, {"NS", 6}};
    std::vector<std::string> blocks(2), counts(2);
    std::string want, want_tagged;
    for (int r = 0; r < 2; ++r) {
        const std::string sh = shared(r), r0 = row(0, r), r1 = row(1, r);
        bcf_put_u32(blocks[0], (uint32_t)sh.size());
        blocks[0] += sh;
        bcf_put_u32(blocks[0], (uint32_t)r0.size());
        blocks[0] += r0;
        bcf_put_u32(blocks[1], (uint32_t)r1.size());
        blocks[1] += r1;
        const uint32_t ac0[2] = {3, 1}, ac1[2] = {1, 1};
        put_site_counts(counts[0], 2, 2, ac0);
        put_site_counts(counts[1], 2, 1, ac1);
        std::string patched = sh, indiv;
        const uint32_t nfs = n_fmt << 24 | n_samples;
        memcpy(&patched[20], &nfs, 4);
        bcf_paste_rows({{(const unsigned char *)r0.data(), r0.size()}, {(const unsigned char *)r1.data(), r1.size()}}, planes, n_fmt, indiv);
        CHECK(r0.size() == 12 && r1.size() == 10 && indiv.size() == 18); // (GQ went to int16 for all three)
        for (int tags = 0; tags < 2; ++tags) {
            std::string &out = tags ? want_tagged : want;
            if (tags) {
                const uint32_t ac[2] = {4, 2};
                bcf_put_info(patched, 0, hdr, ac, 2, 3);
            }
            bcf_put_u32(out, (uint32_t)patched.size());
            bcf_put_u32(out, (uint32_t)indiv.size());
            out += patched + indiv;
        }
    }
    CHECK(want_tagged.size() > want.size());
    auto paste = [&](const std::vector<std::string> &contents, bool tags, bool bgzf) {
        std::deque<PartFile> files, count_files;
        fill(files, base, contents);
        fill(count_files, base + ".cnt", counts);
        SiteCountsReader reader(count_files);
        GroupFiles in;
        in.open(files);
        std::string out;
        paste_bcf_groups(in.f, planes, n_fmt, n_samples, hdr, tags ? &reader : nullptr, bgzf, [&](const char *data, size_t n) { out.append(data, n); });
        return out;
    };
    CHECK(paste(blocks, false, false) == want);
    CHECK(paste(blocks, true, false) == want_tagged);
    for (int tags = 0; tags < 2; ++tags) {
        std::string last;
        CHECK(inflate_bgzf(paste(blocks, tags != 0, true), last) == (tags ? want_tagged : want) && last == bgzf_eof());
    }
    const char *short_file = "a group's block of the merged output is short";
    std::vector<std::string> bad = blocks;
    bad[1].resize(bad[1].size() - 3); // the second group's file ends inside its second row
    CHECK(has(error_of([&]() { paste(bad, false, false); }), short_file));
    bad = blocks;
    bad[0].resize(bad[0].size() - row(0, 1).size() - 4 - 5); // the first group's inside the second shared block
    CHECK(has(error_of([&]() { paste(bad, false, true); }), short_file));
    bad = blocks;
    bad[1].resize(4 + row(1, 0).size()); // no second record at all
    CHECK(has(error_of([&]() { paste(bad, false, false); }), short_file));
    CHECK(has(error_of([&]() {
              std::deque<PartFile> files;
              fill(files, base, {blocks[0]});
              GroupFiles in;
              in.open(files);
              paste_bcf_groups(in.f, planes, n_fmt, n_samples, hdr, nullptr, false, [](const char *, size_t) {});
          }), "their files disagree"));
    CHECK(!exists(base + ".g0.part") && !exists(base + ".cnt.g1.part"));
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    check_part_file(dir);
    check_tables();
    check_site_counts(dir);
    check_pack_stream(dir);
    check_paste_text(dir);
    check_paste_bcf(dir);
    std::cout << "cohort_out_host_check: ok\n";
    return 0;
}
