// Test driver: runs the C++ host's makeSphereTriMesh (host/mesh.cpp) for every record of a binary file -- origin[3], radius as
// binary32, subdivLongitude as uint32 -- and writes positions, normals, indices of each mesh to stdout, raw.  No GPU is touched.
// Built by tests/test_reference_scene.py against host/mesh.cpp and the C-ABI library.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "scene.hpp"

int main(int argc, char* argv[])
{
    if (argc != 2) { std::fprintf(stderr, "usage: host_mesh cases.bin\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 1; }
    unsigned char rec[20];
    while (std::fread(rec, 1, sizeof rec, f) == sizeof rec) {
        float v[4];
        uint32_t subdiv;
        std::memcpy(v, rec, 16);
        std::memcpy(&subdiv, rec + 16, 4);
        const spt_host::TriMesh m = spt_host::makeSphereTriMesh(spt_host::make_float3(v[0], v[1], v[2]), v[3], subdiv);
        std::fwrite(m.positionBuffer.data(), sizeof(m.positionBuffer[0]), m.positionBuffer.size(), stdout);
        std::fwrite(m.normalBuffer.data(), sizeof(m.normalBuffer[0]), m.normalBuffer.size(), stdout);
        std::fwrite(m.indexBuffer.data(), sizeof(uint32_t), m.indexBuffer.size(), stdout);
    }
    std::fclose(f);
    return 0;
}
