// The text form of the batches' render queue tags that sailor_rt_set_scene_tags takes: the tags of the batches in order, separated by commas; an empty field is
// an untagged batch ("Opaque,Masked,,Masked").  Plain C++ without the runtime, so that a stand-alone program can run it under the sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#define SAILOR_RT_BATCH_ALPHA_CUTOUT 1u
#define SAILOR_RT_BATCH_DOUBLE_SIDED 2u
#define SAILOR_RT_TAG_MAX 64u

// -> false (and `out` empty) unless the text has exactly `count` fields, each of at most SAILOR_RT_TAG_MAX letters, digits or underscores.
// A null text stands for `count` empty fields.
inline bool sailor_rt_parse_scene_tags(const char* text, int count, std::vector<std::string>& out)
{
    out.clear();
    if (count < 0) return false;
    if (!text) { out.assign((size_t)count, std::string()); return true; }
    if (count == 0) return *text == 0;
    std::string field;
    for (const char* p = text;; p++) {
        const char c = *p;
        if (c == ',' || c == 0) {
            if (out.size() == (size_t)count) { out.clear(); return false; } // more fields than batches
            out.push_back(field);
            field.clear();
            if (c == 0) break;
            continue;
        }
        const bool ok = (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_';
        if (!ok || field.size() >= SAILOR_RT_TAG_MAX) { out.clear(); return false; }
        field.push_back(c);
    }
    if (out.size() != (size_t)count) { out.clear(); return false; }
    return true;
}

// the shader of one batch, as sailor_rt_set_scene_shaders takes it
#define SAILOR_RT_SHADER_STANDARD 0u
#define SAILOR_RT_SHADER_STANDARD_GLTF 1u
inline bool sailor_rt_scene_shaders_ok(const uint32_t* shaders, int count)
{
    if (count < 0 || (count > 0 && !shaders)) return false;
    for (int i = 0; i < count; i++)
        if (shaders[i] != SAILOR_RT_SHADER_STANDARD && shaders[i] != SAILOR_RT_SHADER_STANDARD_GLTF) return false;
    return true;
}

// the flags of one batch: only the two known bits
inline bool sailor_rt_scene_flags_ok(const uint32_t* flags, int count)
{
    if (count < 0 || (count > 0 && !flags)) return false;
    for (int i = 0; i < count; i++)
        if (flags[i] & ~(SAILOR_RT_BATCH_ALPHA_CUTOUT | SAILOR_RT_BATCH_DOUBLE_SIDED)) return false;
    return true;
}

// the blend mode (EBlendMode: None 0, Additive 1, AlphaBlending 2, Multiply 3 -- Multiply is a known mode; the pass that draws it is refused) and the z-write
// flag (0 or 1) of one batch, as sailor_rt_set_scene_blend takes them
inline bool sailor_rt_scene_blend_ok(const uint32_t* blendModes, const uint32_t* zWrite, int count)
{
    if (count < 0 || (count > 0 && (!blendModes || !zWrite))) return false;
    for (int i = 0; i < count; i++)
        if (blendModes[i] > 3u || zWrite[i] > 1u) return false;
    return true;
}
