// tools/newick_host_check.cpp -- the Newick reader (skh_newick_joins, ska.rust_amd/host/ska_tree.cpp) on its own, fed what a user's
// file may hold: well-formed trees, every truncation of them, nesting far deeper than a call stack, caterpillars, a list of malformed texts and
// some ten thousand random edits of good ones.  Every text is handed over in a heap block of exactly its length + 1, so that a sanitizer sees a
// read past its end; a text the reader takes must come back as a join table that is a tree, one it refuses as SKX_EINVAL with a "newick:" message.
// The two writers are run on every table the reader returns.  No device and no libskx.so: the file is compiled together with ska_tree.cpp.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o newick_host_check tools/newick_host_check.cpp ska.rust_amd/host/ska_tree.cpp
//   ./newick_host_check          prints the counts; exit code 0 when everything held
#include "../include/skx_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::string g_error;
extern "C" void skx_set_last_error(const char *msg) { g_error = msg ? msg : ""; }
extern "C" void skx_free(void *p) { free(p); }

static unsigned long long taken = 0, refused = 0, failures = 0;

static void fail(const char *what, const std::string &text)
{
    failures++;
    fprintf(stderr, "FAILED: %s: %.120s%s\n", what, text.c_str(), text.size() > 120 ? "..." : "");
}

// 1: taken, 0: refused
static int feed(const std::string &text, const std::vector<std::string> &names)
{
    const int n = (int)names.size();
    std::vector<const char *> cn;
    for (auto &s : names) cn.push_back(s.c_str());
    char *exact = (char *)malloc(text.size() + 1);
    memcpy(exact, text.c_str(), text.size() + 1);
    std::vector<skx_tree_join> joins((size_t)n - 1, skx_tree_join{0xFFFFFFFFu, 0xFFFFFFFFu});
    int three = -1;
    g_error.clear();
    const int r = skh_newick_joins(exact, cn.data(), n, joins.data(), &three);
    free(exact);
    if (r == SKX_EINVAL) {
        if (g_error.compare(0, 7, "newick:") != 0) fail("a refusal without its message", text);
        refused++;
        return 0;
    }
    if (r != SKX_OK) { fail("an unexpected return code", text); return 0; }
    std::vector<char> used(2 * (size_t)n - 1, 0);
    for (int t = 0; t + 1 < n; t++)
        for (const uint32_t c : {joins[t].a, joins[t].b}) {
            if (c >= (uint32_t)(n + t) || used[c]) { fail("a table that is not a tree", text); return 1; }
            used[c] = 1;
        }
    if (three != 0 && three != 1) fail("root_three not set", text);
    std::vector<uint64_t> changes(2 * (size_t)n - 2);
    for (size_t i = 0; i < changes.size(); i++) changes[i] = i * 7 % 1000;
    for (auto writer : {skh_parsimony_newick, skh_parsimony_branches}) {
        char *buf = nullptr; uint64_t len = 0;
        if (writer(cn.data(), joins.data(), n, three, changes.data(), &buf, &len) != SKX_OK || !buf || strlen(buf) != len) fail("a writer refused the reader's table", text);
        if (writer == skh_parsimony_newick && buf) {                   // what was written reads back as the same table
            std::vector<skx_tree_join> again((size_t)n - 1);
            int three2 = -1;
            if (skh_newick_joins(buf, cn.data(), n, again.data(), &three2) != SKX_OK || three2 != three || memcmp(again.data(), joins.data(), again.size() * sizeof(skx_tree_join)) != 0)
                fail("the written tree does not read back", text);
        }
        free(buf);
    }
    taken++;
    return 1;
}

int main()
{
    const std::vector<std::string> four = {"a", "b c", "it's", "d"};
    const std::vector<std::string> good = {
        "((a,'b c'),('it''s',d));", " ( (a:1 , 'b c'[x]:2e-1)'l''1':0.5,('it''s',d)[y]:3 ) ; ", "(a,'b c',('it''s',d));", "((a,'b c'):1,'it''s':2,d:3)root;",
        "(a:0.1,('b c':0.2,('it''s':0.3,d:0.4)90:0.5)80:0.6);", "[c]((a,[c]'b c')[c],[c]('it''s',d)[c])[c];[c]",
    };
    for (auto &t : good) {
        if (!feed(t, four)) fail(("a good text was refused: " + g_error).c_str(), t);
        for (size_t cut = 0; cut < t.size(); cut++) feed(t.substr(0, cut), four);      // (a cut behind the ';' may still be a tree)
    }
    const std::vector<std::string> malformed = {
        "", ";", "()", "();", "(,);", "(a);", "((a,'b c',d),'it''s');", "(a,'b c','it''s',d);", "((a,'b c'),('it''s',x));", "((a,'b c'),('it''s',a));", "((a,'b c'),d);",
        "((a,'b c'),('it''s',d)); x", "((a,'b c'),('it''s',d)))", "((a,'b c'),('it''s,d));", "((a,'b c'),[('it''s',d));", "((a,'b c')('it''s',d));", "((a 'b c'),('it''s',d));",
        "((a,,'b c'),('it''s',d));", ")(", "'", "''", "[", "]", ":", ":::", "(((((((((", ")))))))))", "a;", "a,b;", "(a,'b c'),('it''s',d);", "((a,'b c'),('it''s',d)):;", "((a,'b c'),('it''s',d))::;",
        "((a:,'b c':),('it''s':,d:):):;", "((a,'b c'),('it''s',d));;", "(('b c',a),(d,'it''s'))\x01;", "((a,\xff),('it''s',d));",
    };
    for (auto &t : malformed) feed(t, four);
    // nesting no call stack would survive, open and closed
    for (const size_t depth : {(size_t)1000, (size_t)300000}) {
        feed(std::string(depth, '('), four);
        feed(std::string(depth, '(') + "a" + std::string(depth, ')') + ";", four);
        feed(std::string(depth, '(') + std::string(depth, ')') + ";", four);
        feed(std::string(depth, '[') + ";", four);
        feed(std::string(depth, '\'') + ";", four);
    }
    // caterpillars nested on the left and on the right, and one leaf too many
    for (const int n : {2, 3, 1000, 60000}) {
        std::vector<std::string> names;
        for (int i = 0; i < n; i++) names.push_back("s" + std::to_string(i));
        std::string left = std::string((size_t)n - 1, '(') + names[0], right;
        for (int i = 1; i < n; i++) left += "," + names[i] + "):" + std::to_string(i);
        for (int i = 0; i + 1 < n; i++) right += "(" + names[i] + ",";
        right += names[n - 1] + std::string((size_t)n - 1, ')');
        if (!feed(left + ";", names) || !feed(right + ";", names)) fail(("a caterpillar was refused: " + g_error).c_str(), std::to_string(n));
        feed("(" + left + ",extra);", names);
        feed(left, names);
    }
    // random edits of the good texts: bytes replaced, dropped, doubled
    unsigned long long x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    static const char alphabet[] = "()[]':;, ab'c\t\n01.e-";
    for (int round = 0; round < 12000; round++) {
        std::string t = good[next() % good.size()];
        for (int edits = 1 + (int)(next() % 3); edits-- && !t.empty();) {
            const size_t at = next() % t.size();
            switch (next() % 3) {
            case 0: t[at] = alphabet[next() % (sizeof alphabet - 1)]; break;
            case 1: t.erase(at, 1); break;
            default: t.insert(at, 1, t[at]); break;
            }
        }
        feed(t, four);
    }
    printf("newick_host_check: %llu texts taken, %llu refused, %llu failures\n", taken, refused, failures);
    return failures ? 1 : 0;
}
