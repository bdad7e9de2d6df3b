// Driver for tests/golden/make_cubed_sphere_case.py: runs the reference's cubed-sphere halo
// generator, its tile transforms and its seven-argument intersect on a set of configurations
// and prints what they produce as JSON. Compiled by hand against the GHEX v0.8.0 headers (plus
// an include directory holding an empty ghex/config.hpp); never built or run by a test.
//
// Input (stdin): n_configs, then per configuration: edge_size levels h0 h1 h2 h3 n_domains, then
// per domain: tile x_first x_last y_first y_last.
#include <ghex/structured/cubed_sphere/halo_generator.hpp>

#include <cstdio>
#include <iostream>
#include <vector>

using namespace ghex::structured::cubed_sphere;

int main()
{
    int n_cfg = 0;
    std::cin >> n_cfg;
    std::printf("[");
    for (int q = 0; q < n_cfg; ++q)
    {
        int c, levels, h[4], nd;
        std::cin >> c >> levels >> h[0] >> h[1] >> h[2] >> h[3] >> nd;
        std::vector<domain_descriptor> doms;
        for (int i = 0; i < nd; ++i)
        {
            int t, xf, xl, yf, yl;
            std::cin >> t >> xf >> xl >> yf >> yl;
            doms.emplace_back(cube{c, levels}, t, xf, xl, yf, yl);
        }
        std::array<int, 4> ha{h[0], h[1], h[2], h[3]};
        halo_generator     gen(ha);
        std::printf("%s{\"edge_size\":%d,\"levels\":%d,\"halos\":[%d,%d,%d,%d],\"domains\":[",
            q ? "," : "", c, levels, h[0], h[1], h[2], h[3]);
        for (int i = 0; i < nd; ++i)
        {
            const auto& d = doms[i];
            std::printf("%s{\"tile\":%d,\"x\":[%d,%d],\"y\":[%d,%d],\"boxes\":[", i ? "," : "",
                d.domain_id().tile, d.first()[1], d.last()[1], d.first()[2], d.last()[2]);
            const auto boxes = gen(d);
            bool       first_box = true;
            for (const auto& b : boxes)
            {
                const int        tile = b.global().first()[0];
                const transform* t = &identity_transform;
                if (tile != d.domain_id().tile)
                {
                    int n;
                    for (n = 0; n < 4; ++n)
                        if (tile_lu[d.domain_id().tile][n] == tile) break;
                    t = &transform_lu[d.domain_id().tile][n];
                }
                const int lx = b.local().first()[1], ly = b.local().first()[2];
                const int gx = lx + d.first()[1], gy = ly + d.first()[2];
                const auto p0 = (*t)(gx, gy, c), p1 = (*t)(gx + 1, gy, c), p2 = (*t)(gx, gy + 1, c);
                std::printf("%s{\"l\":[%d,%d,%d,%d,%d,%d],\"g\":[%d,%d,%d,%d,%d,%d],\"t\":%d,"
                            "\"img\":[%d,%d,%d,%d,%d,%d],\"sign\":[%d,%d],\"x\":[",
                    first_box ? "" : ",", b.local().first()[1], b.local().first()[2],
                    b.local().first()[3], b.local().last()[1], b.local().last()[2],
                    b.local().last()[3], b.global().first()[1], b.global().first()[2],
                    b.global().first()[3], b.global().last()[1], b.global().last()[2],
                    b.global().last()[3], tile, p0[0], p0[1], p1[0], p1[1], p2[0], p2[1],
                    t->m_rotation[2] == -1 ? -1 : 1, t->m_rotation[1] == -1 ? -1 : 1);
                first_box = false;
                bool first_x = true;
                for (int j = 0; j < nd; ++j)
                {
                    const auto& o = doms[j];
                    const auto  x = gen.intersect(d, b.local().first(), b.local().last(),
                         b.global().first(), b.global().last(), o.first(), o.last());
                    if (!(x.global().first() <= x.global().last())) continue;
                    std::printf("%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d]", first_x ? "" : ",", j,
                        x.local().first()[1], x.local().first()[2], x.local().first()[3],
                        x.local().last()[1], x.local().last()[2], x.local().last()[3],
                        x.global().first()[1], x.global().first()[2], x.global().first()[3],
                        x.global().last()[1], x.global().last()[2], x.global().last()[3]);
                    first_x = false;
                }
                std::printf("]}");
            }
            std::printf("]}");
        }
        std::printf("]}");
    }
    std::printf("]\n");
    return 0;
}
