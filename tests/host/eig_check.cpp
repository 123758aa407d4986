// Host-side check of csrc/fdyn_eig.hpp, the 4 x 4 eigenvalue solver and mode summary the flight-modes kernel compiles: built with
// the host compiler under AddressSanitizer and UBSan, never launched on a device.
//   in   fp64 words: n, then n x { m [4][4] }
//   out  fp64 words: n x { re [4], im [4], summary [FD_NMO], sweeps, ok }
// The test compares the output with the NumPy model bit for bit.  Exit status 0 when both files were read and written whole.
#include <stdio.h>
#include <vector>
#include "../../hybrid-classical-and-reinforcement-learning-aircraft-controllers_amd/csrc/fdyn_eig.hpp"

using namespace fdyn;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    double head;
    if (!f || fread(&head, sizeof(double), 1, f) != 1) return 3;
    const size_t n = size_t(head), words = n * 16;
    std::vector<double> in(words), out;
    if (fread(in.data(), sizeof(double), words, f) != words) return 3;
    fclose(f);
    for (size_t k = 0; k < n; ++k) {
        double m[EIG_N][EIG_N], re[EIG_N], im[EIG_N], s[FD_NMO];
        for (int r = 0; r < EIG_N; ++r)
            for (int c = 0; c < EIG_N; ++c) m[r][c] = in[k * 16 + r * EIG_N + c] + 0.0;
        int sweeps;
        const bool ok = eig4(m, re, im, sweeps);
        mode_summary(re, im, s);
        out.insert(out.end(), re, re + EIG_N);
        out.insert(out.end(), im, im + EIG_N);
        out.insert(out.end(), s, s + FD_NMO);
        out.push_back(double(sweeps));
        out.push_back(ok ? 1.0 : 0.0);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    fclose(f);
    printf("solved %zu matrices\n", n);
    return 0;
}
