// C entry points that let the Python test-suite drive the C++ host mirror exactly the way the engine would:
// create the renderer (HIP backend), build a frame graph BY NODE NAME, hand it a scene snapshot, process frames, read back.
#include <memory>
#include <string>
#include "Runtime/ECS/LightingECS.h"
#include "Runtime/FrameGraph/LightCullingNode.h"
#include "Runtime/FrameGraph/DepthPrepassNode.h"
#include "Runtime/FrameGraph/ParticlesNode.h"
#include "Runtime/FrameGraph/RHIFrameGraph.h"
#include "Runtime/GraphicsDriver/HIP/HipGraphicsDriver.h"
#include "Runtime/RHI/Renderer.h"
#include "Runtime/RHI/DebugContext.h"
#include "Runtime/AssetRegistry/FrameGraph/FrameGraphParser.h"
#include "Runtime/AssetRegistry/World/WorldPrefabImporter.h"
#include "scene_tags.h"
#include <algorithm>
#include <cstdio>
#include <vector>

using namespace Sailor;
using namespace Sailor::RHI;
using namespace Sailor::Framegraph;

#define RT_API extern "C" __attribute__((visibility("default")))

struct SailorRuntime {
    std::unique_ptr<Renderer> renderer;
    std::unique_ptr<LightingECS> lighting;
    RHIFrameGraph graph;
    RHISceneViewSnapshot snapshot;
    FrameGraphNodePtr lightCulling, renderScene, linearizeDepth, environment;
    std::vector<FrameGraphNodePtr> queueNodes; // the RenderScene nodes sailor_rt_build_graph created with a queue ("RenderScene:Masked"): they get the scene's targets too
    RHITexturePtr depthHighZ;
    RHITexturePtr depth, rawDepth;
    RHIBufferPtr surface, radiance;
    std::unique_ptr<EcsSweepSystem> sweep;
    DebugContext debug; // the world's DebugContext (Engine/World.h): the snapshot points at it
    RHIImGuiDrawData ui; // the frame's ImDrawData and ImGuiApi's backend data: the snapshot points at it while there is draw data
    int frames = 0;
    std::vector<long long> captureBytes; // sailor_rt_capture_next_frame: [slot][name] bytes copied, -1 absent, -2 larger than its capacity
    int captureSlots = 0;
};

RT_API SailorRuntime* sailor_rt_create(int device, void* stream, int ownStream, int* outStatus)
{
    auto* rt = new SailorRuntime();
    rt->renderer.reset(new Renderer(device, stream, ownStream != 0));
    if (outStatus) *outStatus = rt->renderer->GetStatus();
    if (rt->renderer->GetStatus() != SAILOR_HIP_OK) { delete rt; return nullptr; }
    rt->lighting.reset(new LightingECS());
    rt->snapshot.m_debugContext = &rt->debug;
    return rt;
}

RT_API void sailor_rt_destroy(SailorRuntime* rt)
{
    if (!rt) return;
    Renderer::GetDriver()->WaitIdle();
    rt->graph.Clear();
    rt->sweep.reset();
    rt->lighting.reset();
    rt->debug.Clear();
    rt->snapshot.m_drawImGui = nullptr;
    rt->ui = RHIImGuiDrawData();
    rt->depth.Clear(); rt->surface.Clear(); rt->radiance.Clear(); rt->depthHighZ.Clear();
    rt->lightCulling.Clear(); rt->renderScene.Clear(); rt->linearizeDepth.Clear(); rt->environment.Clear(); rt->rawDepth.Clear();
    rt->queueNodes.clear();
    rt->snapshot = RHISceneViewSnapshot();
    delete rt;
}

RT_API int sailor_rt_node_registered(const char* name) { return FrameGraphBuilder::IsRegistered(name) ? 1 : 0; }

// Opt this runtime's graphs in to a node class that is compiled in but not registered (FrameGraphBuilder::CreateOptInNode: "Bloom"): sailor_rt_load_renderer
// and sailor_rt_build_graph then create it where they meet the name; sailor_rt_node_registered keeps answering 0, and a runtime that did not opt in
// keeps skipping the entry.  In the engine the class registers normally (BloomNode.h:43); the opt-in exists because this mirror's older tests use "Bloom" as
// their example of a name without a node class.  0, or -1 for a name that has no such class.
RT_API int sailor_rt_enable_node(SailorRuntime* rt, const char* name)
{
    if (!rt || !name || !FrameGraphBuilder::CreateOptInNode(name)) return -1;
    rt->graph.EnableNode(name);
    return 0;
}

// Opt this runtime's driver in to a shader that has an entry point but is not routed by default: "Shaders/MotionBlur.shader" or "Shaders/Debug.shader" (the
// frame's tail), "Shaders/Stars.shader" or "Shaders/SunShafts.shader" (the Sky node's star points and sun shafts; before the first frame, when the node
// creates its shaders).  PostProcess nodes created afterwards find the shader ready and draw with it; a runtime that did not opt in keeps creating it "not ready",
// so its nodes record nothing, and sailor_rt_enable_node("MotionBlur") keeps failing: there is no such node class.  In the engine the backend would simply route
// both; as with Bloom, the opt-in exists only because this mirror's older tests use MotionBlur.shader as their example of a shader without an entry point.
// 0, or -1 for any other path or a null runtime.
RT_API int sailor_rt_enable_shader(SailorRuntime* rt, const char* path)
{
    if (!rt || !path || !rt->renderer) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    return hip && hip->EnableShader(path) ? 0 : -1;
}

// builds the graph from node names, as FrameGraphImporter does from the .renderer YAML (FrameGraphParser.cpp:153)
RT_API int sailor_rt_build_graph(SailorRuntime* rt, const char** nodeNames, int count)
{
    for (int i = 0; i < count; i++) {
        // "RenderScene:<Tag>" is a RenderScene node with that `Tag` (DefaultRenderer.renderer lists RenderScene twice: `Tag: Opaque`, then `Tag: Masked`)
        if (std::string(nodeNames[i]).rfind("RenderScene:", 0) == 0) {
            auto queue = FrameGraphBuilder::CreateNode("RenderScene");
            if (!queue) return -1;
            queue->SetString("Tag", nodeNames[i] + 12);
            rt->queueNodes.push_back(queue);
            rt->graph.AddNode(queue);
            continue;
        }
        auto node = FrameGraphBuilder::CreateNode(nodeNames[i]);
        if (!node && rt->graph.IsNodeEnabled(nodeNames[i])) node = FrameGraphBuilder::CreateOptInNode(nodeNames[i]);
        if (!node) return -1;
        if (std::string(nodeNames[i]) == "LightCulling") rt->lightCulling = node;
        if (std::string(nodeNames[i]) == "LinearizeDepth") rt->linearizeDepth = node;
        if (std::string(nodeNames[i]) == "Environment") rt->environment = node;
        if (std::string(nodeNames[i]) == "RenderScene") { node->SetString("Tag", "Opaque"); rt->renderScene = node; }
        rt->graph.AddNode(node);
    }
    return 0;
}

// FrameGraphAsset::Deserialize alone (no device): a one-line summary of what a `.renderer` text declares, for the CPU tests:
//   "targets=Name:WxH:format:mips,...;nodes=Name[tag]{string k=v;float k=v;vec4 k=x y z w;rt k=v},...;values=k=v,...;samplers=a,b"
// WorldPrefab::Deserialize + World::Instantiate of a `.world` text (no device needed): a one-line summary for the tests, -1 + message on an error
static std::string world_summary(const WorldScene& scene)
{
    char b[768];
    std::string s = "name=" + scene.m_name + ";objects=" + std::to_string(scene.m_gameObjects.size()) + ";";
    for (const auto& go : scene.m_gameObjects) {
        snprintf(b, sizeof b, "%s[parent=%d pos=%g %g %g rot=%.9g %.9g %.9g %.9g scale=%g %g %g comps=", go.m_name.c_str(), (int)go.m_parent, go.m_transform.position[0],
                 go.m_transform.position[1], go.m_transform.position[2], go.m_transform.rotation[0], go.m_transform.rotation[1], go.m_transform.rotation[2],
                 go.m_transform.rotation[3], go.m_transform.scale[0], go.m_transform.scale[1], go.m_transform.scale[2]);
        s += b;
        for (size_t i = 0; i < go.m_componentTypes.size(); i++) s += (i ? "," : "") + go.m_componentTypes[i];
        s += "];";
    }
    for (const auto& c : scene.m_cameras) {
        snprintf(b, sizeof b, "camera{owner=%u fov=%g zNear=%g zFar=%g};", c.m_owner, c.m_fov, c.m_zNear, c.m_zFar);
        s += b;
    }
    for (const auto& l : scene.m_lights) {
        snprintf(b, sizeof b, "light{owner=%u type=%u intensity=%g %g %g attenuation=%.9g %.9g %.9g bounds=%g %g %g cutOff=%g %g dir=%.9g %.9g %.9g pos=%g %g %g};", l.m_owner,
                 (unsigned)l.m_data.m_type, l.m_data.m_intensity[0], l.m_data.m_intensity[1], l.m_data.m_intensity[2], l.m_data.m_attenuation[0], l.m_data.m_attenuation[1],
                 l.m_data.m_attenuation[2], l.m_data.m_bounds[0], l.m_data.m_bounds[1], l.m_data.m_bounds[2], l.m_data.m_cutOff[0], l.m_data.m_cutOff[1], l.m_data.m_direction[0],
                 l.m_data.m_direction[1], l.m_data.m_direction[2], l.m_data.m_worldPosition[0], l.m_data.m_worldPosition[1], l.m_data.m_worldPosition[2]);
        s += b;
    }
    for (const auto& m : scene.m_meshRenderers) s += "mesh{owner=" + std::to_string(m.m_owner) + " model=" + m.m_modelFileId + "};";
    s += "other=" + std::to_string(scene.m_otherComponents);
    return s;
}

RT_API int sailor_rt_parse_world(const char* yamlText, char* out, int outSize)
{
    WorldPrefab prefab;
    WorldScene scene;
    std::string err;
    if (!prefab.Deserialize(yamlText ? yamlText : "", &err) || !scene.Instantiate(prefab, &err)) {
        if (out && outSize > 0) snprintf(out, (size_t)outSize, "error: %s", err.c_str());
        return -1;
    }
    if (out && outSize > 0) snprintf(out, (size_t)outSize, "%s", world_summary(scene).c_str());
    return (int)scene.m_gameObjects.size();
}

// Loads a `.world` into the runtime the way Sailor.cpp:185-190 + World::Instantiate do for the parts the path reads: the first camera becomes the scene view's
// camera (aspect from the viewport), every LightComponent registers with the lighting system and is packed by LightingECS::Tick, and the game objects' transforms /
// parent indices come back flat for the ECS sweep (outTransforms: 12 floats each, outParents; up to maxObjects).  Returns the number of game objects.
RT_API int sailor_rt_load_world(SailorRuntime* rt, const char* yamlText, int width, int height, float* outTransforms, uint32_t* outParents, int maxObjects, int* outLights,
                                int* outMeshes)
{
    WorldPrefab prefab;
    WorldScene scene;
    if (!prefab.Deserialize(yamlText ? yamlText : "") || !scene.Instantiate(prefab)) return -1;
    if (!scene.m_cameras.empty()) {
        const auto& c = scene.m_cameras[0];
        memcpy(rt->snapshot.m_camera.m_world, scene.m_gameObjects[c.m_owner].m_world, 64);
        rt->snapshot.m_camera.m_fov = c.m_fov; rt->snapshot.m_camera.m_aspect = (float)width / (float)height;
        rt->snapshot.m_camera.m_zNear = c.m_zNear; rt->snapshot.m_camera.m_zFar = c.m_zFar;
    }
    rt->graph.SetViewport(width, height);
    for (const auto& l : scene.m_lights) rt->lighting->RegisterComponent(l.m_data);
    auto cmd = Renderer::GetDriver()->CreateCommandList();
    rt->lighting->Tick(cmd);
    Renderer::GetDriver()->SubmitCommandList(cmd);
    rt->lighting->FillLightingData(rt->snapshot);
    for (int i = 0; i < (int)scene.m_gameObjects.size() && i < maxObjects; i++) {
        if (outTransforms) memcpy(outTransforms + 12 * i, &scene.m_gameObjects[i].m_transform, 48);
        if (outParents) outParents[i] = scene.m_gameObjects[i].m_parent;
    }
    if (outLights) *outLights = (int)scene.m_lights.size();
    if (outMeshes) *outMeshes = (int)scene.m_meshRenderers.size();
    return (int)scene.m_gameObjects.size();
}

RT_API int sailor_rt_parse_renderer(const char* yamlText, int viewportWidth, int viewportHeight, char* out, int outSize)
{
    FrameGraphAsset asset;
    std::string err;
    if (!asset.Deserialize(yamlText ? yamlText : "", viewportWidth, viewportHeight, &err)) {
        if (out && outSize > 0) snprintf(out, (size_t)outSize, "error: %s", err.c_str());
        return -1;
    }
    std::string s = "targets=";
    for (size_t i = 0; i < asset.m_renderTargets.size(); i++) {
        const auto& t = asset.m_renderTargets[i];
        const uint32_t maxExtent = t.m_width > t.m_height ? t.m_width : t.m_height;
        uint32_t mips = 1;
        if (t.m_bGenerateMips) { mips = 0; for (uint32_t e = maxExtent; e; e >>= 1) mips++; }
        if (mips > t.m_maxMipLevel) mips = t.m_maxMipLevel;
        s += (i ? "," : "") + t.m_name + ":" + std::to_string(t.m_width) + "x" + std::to_string(t.m_height) + ":" + t.m_format + ":" + std::to_string(mips) +
             (t.m_reduction != "Average" ? ":" + t.m_reduction : "");
    }
    s += ";nodes=";
    for (size_t i = 0; i < asset.m_nodes.size(); i++) {
        const auto& n = asset.m_nodes[i];
        s += (i ? "," : "") + n.m_name + "[" + n.m_tag + "]{";
        for (const auto& p : n.m_strings) s += "string " + p.first + "=" + p.second + ";";
        for (const auto& p : n.m_floats) { char b[64]; snprintf(b, sizeof b, "%g", p.second); s += "float " + p.first + "=" + b + ";"; }
        for (const auto& p : n.m_vectors) { char b[128]; snprintf(b, sizeof b, "%g %g %g %g", p.second.x, p.second.y, p.second.z, p.second.w); s += "vec4 " + p.first + "=" + b + ";"; }
        for (const auto& p : n.m_renderTargets) s += "rt " + p.first + "=" + p.second + ";";
        s += "}";
    }
    s += ";values=";
    { bool first = true; for (const auto& v : asset.m_values) { char b[64]; snprintf(b, sizeof b, "%g", v.second); s += (first ? "" : ",") + v.first + "=" + b; first = false; } }
    s += ";samplers=";
    for (size_t i = 0; i < asset.m_samplers.size(); i++) s += (i ? "," : "") + asset.m_samplers[i];
    if (out && outSize > 0) snprintf(out, (size_t)outSize, "%s", s.c_str());
    return (int)asset.m_nodes.size();
}

// FrameGraphImporter: build the runtime's frame graph from a `.renderer` text -- render targets, values, one node per `frame` entry that has a
// node class here (the others are reported, as the reference logs them).  Returns the number of nodes created, < 0 on a parse error.
RT_API int sailor_rt_load_renderer(SailorRuntime* rt, const char* yamlText, int* outNotImplemented, int* outRenderTargets)
{
    FrameGraphAsset asset;
    if (!asset.Deserialize(yamlText ? yamlText : "", rt->graph.GetViewport().x, rt->graph.GetViewport().y)) return -1;
    rt->graph.Clear();
    rt->lightCulling.Clear(); rt->renderScene.Clear(); rt->linearizeDepth.Clear(); rt->environment.Clear();
    rt->queueNodes.clear();
    const FrameGraphBuildReport report = FrameGraphImporter::BuildFrameGraph(asset, rt->graph);
    for (const auto& node : rt->graph.GetGraph()) { // the harness' setters address these nodes directly
        const std::string name = node->GetDebugName();
        if (name == "LightCulling") rt->lightCulling = node;
        if (name == "LinearizeDepth") rt->linearizeDepth = node;
        if (name == "Environment") rt->environment = node;
        if (name == "RenderScene" && !rt->renderScene) rt->renderScene = node;
    }
    if (rt->renderScene && rt->surface) { rt->renderScene->SetRHIResource("surface", rt->surface); rt->renderScene->SetRHIResource("radiance", rt->radiance); }
    if (outNotImplemented) *outNotImplemented = report.m_nodesNotImplemented;
    if (outRenderTargets) *outRenderTargets = report.m_renderTargets;
    return report.m_nodesCreated;
}

// a render target of the loaded graph, by the name the `.renderer` text gives it
RT_API void* sailor_rt_render_target(SailorRuntime* rt, const char* name, int* outWidth, int* outHeight, int* outLevels)
{
    auto t = rt->graph.GetRenderTarget(name);
    if (!t || !t->m_buffer) return nullptr;
    if (outWidth) *outWidth = t->GetExtent().x;
    if (outHeight) *outHeight = t->GetExtent().y;
    if (outLevels) *outLevels = (int)t->GetMipLevels();
    return t->m_buffer->m_hip.m_devicePtr;
}

// publish a wrapped device image as a named render target of the graph (the per-frame targets a `.renderer` file leaves unresolved: DepthBuffer, ...)
RT_API void sailor_rt_set_render_target(SailorRuntime* rt, const char* name, void* devicePtr, int width, int height)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    rt->graph.SetRenderTarget(name, hip->WrapTexture(devicePtr, { width, height }, EFormat::R32_SFLOAT));
}

RT_API void sailor_rt_set_camera(SailorRuntime* rt, const float* world16, float fov, float aspect, float zNear, float zFar, int width, int height)
{
    memcpy(rt->snapshot.m_camera.m_world, world16, 64);
    rt->snapshot.m_camera.m_fov = fov; rt->snapshot.m_camera.m_aspect = aspect;
    rt->snapshot.m_camera.m_zNear = zNear; rt->snapshot.m_camera.m_zFar = zFar;
    rt->graph.SetViewport(width, height);
}

// lights: packed LightShaderData records (host memory); goes through UpdateShaderBinding like LightingECS::Tick
RT_API void sailor_rt_set_lights(SailorRuntime* rt, const void* records, int count)
{
    auto cmd = Renderer::GetDriver()->CreateCommandList();
    rt->lighting->SetPacked(cmd, (const SailorLightShaderData*)records, (size_t)count);
    Renderer::GetDriver()->SubmitCommandList(cmd);
    rt->lighting->FillLightingData(rt->snapshot);
}

// lights as components (degrees, defaults of ECS/LightingECS.h:23-28), packed by LightingECS::Tick
RT_API int sailor_rt_add_light(SailorRuntime* rt, uint32_t type, uint32_t shadowType, const float* pos, const float* dir, const float* intensity,
                               const float* bounds, const float* cutOffDegrees)
{
    LightData d;
    d.m_type = (ELightType)type; d.m_shadowType = (EShadowType)shadowType;
    memcpy(d.m_worldPosition, pos, 12); memcpy(d.m_direction, dir, 12); memcpy(d.m_intensity, intensity, 12); memcpy(d.m_bounds, bounds, 12);
    if (cutOffDegrees) memcpy(d.m_cutOff, cutOffDegrees, 8);
    return (int)rt->lighting->RegisterComponent(d);
}

RT_API void sailor_rt_tick_lights(SailorRuntime* rt)
{
    auto cmd = Renderer::GetDriver()->CreateCommandList();
    rt->lighting->Tick(cmd);
    Renderer::GetDriver()->SubmitCommandList(cmd);
    rt->lighting->FillLightingData(rt->snapshot);
}

// LightComponent setters + MarkDirty (Components/LightComponent.h): new parameters for one light; null pointers leave a field alone
RT_API int sailor_rt_update_light(SailorRuntime* rt, int index, const float* pos, const float* dir, const float* intensity, const float* bounds,
                                  const float* cutOffDegrees)
{
    if (!rt || index < 0 || (size_t)index >= rt->lighting->Num()) return -1;
    LightData& d = rt->lighting->GetComponentData((size_t)index);
    if (pos) memcpy(d.m_worldPosition, pos, 12);
    if (dir) memcpy(d.m_direction, dir, 12);
    if (intensity) memcpy(d.m_intensity, intensity, 12);
    if (bounds) memcpy(d.m_bounds, bounds, 12);
    if (cutOffDegrees) memcpy(d.m_cutOff, cutOffDegrees, 8);
    d.m_bIsDirty = true;
    return 0;
}

// What Tick asks of the component and its owner besides the parameters: TComponent::SetActive, MarkDirty, the owner's mobility and the frame
// its transform last changed (GameObject::GetFrameLastChange); a negative value leaves the field alone.
RT_API int sailor_rt_set_light_state(SailorRuntime* rt, int index, int active, int dirty, int mobility, long long ownerFrameLastChange)
{
    if (!rt || index < 0 || (size_t)index >= rt->lighting->Num()) return -1;
    LightData& d = rt->lighting->GetComponentData((size_t)index);
    if (active >= 0) d.m_bIsActive = active != 0;
    if (dirty >= 0) d.m_bIsDirty = dirty != 0;
    if (mobility >= 0) d.m_ownerMobility = (EMobilityType)mobility;
    if (ownerFrameLastChange >= 0) d.m_ownerFrameLastChange = (size_t)ownerFrameLastChange;
    return 0;
}

// the copies the last sailor_rt_tick_lights recorded: (first record slot, record count) pairs in issue order; returns their number
RT_API int sailor_rt_light_uploads(SailorRuntime* rt, uint32_t* outStartCount, int maxRuns)
{
    const auto& runs = rt->lighting->GetLastUploads();
    for (int i = 0; i < (int)runs.size() && i < maxRuns; i++) {
        outStartCount[2 * i] = (uint32_t)runs[(size_t)i].m_startIndex;
        outStartCount[2 * i + 1] = (uint32_t)runs[(size_t)i].m_count;
    }
    return (int)runs.size();
}

RT_API uint32_t sailor_rt_total_num_lights(SailorRuntime* rt) { return rt->snapshot.m_totalNumLights; }

// LightingECS::Tick's loop without a renderer (no device needed): `count` default lights with the given flags, `ticks` passes in a row with the
// skip list carried from pass to pass; a light's position is (its slot, pass, 0).  Per pass: outRunCounts[pass] runs appended to outStartCount
// (pairs), the records of those runs appended to outRecords (112 B each).  Flags are updated in place.  Returns the total number of runs.
RT_API int sailor_rt_plan_light_uploads(int count, uint8_t* dirty, const uint8_t* active, const uint8_t* mobility, uint64_t* frameLastChange,
                                        const uint64_t* ownerFrameLastChange, int ticks, const uint8_t* redirtyPerTick, int* outRunCounts,
                                        uint32_t* outStartCount, int maxRuns, void* outRecords, int maxRecords)
{
    std::vector<LightData> comps((size_t)count);
    for (int i = 0; i < count; i++) {
        comps[(size_t)i].m_bIsDirty = dirty[i] != 0; comps[(size_t)i].m_bIsActive = active[i] != 0;
        comps[(size_t)i].m_ownerMobility = (EMobilityType)mobility[i];
        comps[(size_t)i].m_frameLastChange = (size_t)frameLastChange[i]; comps[(size_t)i].m_ownerFrameLastChange = (size_t)ownerFrameLastChange[i];
    }
    std::vector<std::pair<uint32_t, uint32_t>> skipList;
    int total = 0, totalRecords = 0;
    for (int t = 0; t < ticks; t++) {
        for (int i = 0; i < count; i++) {
            comps[(size_t)i].m_worldPosition[0] = (float)i; comps[(size_t)i].m_worldPosition[1] = (float)t;
            if (t > 0 && redirtyPerTick && redirtyPerTick[(size_t)(t - 1) * count + i]) comps[(size_t)i].m_bIsDirty = true;
        }
        std::vector<SailorLightShaderData> records;
        const auto runs = LightingECS::CollectDirtyRuns(comps, skipList, records);
        outRunCounts[t] = (int)runs.size();
        for (const auto& r : runs) {
            if (total < maxRuns) { outStartCount[2 * total] = (uint32_t)r.m_startIndex; outStartCount[2 * total + 1] = (uint32_t)r.m_count; }
            total++;
        }
        for (const auto& rec : records) {
            if (totalRecords < maxRecords) memcpy((uint8_t*)outRecords + sizeof(SailorLightShaderData) * (size_t)totalRecords, &rec, sizeof rec);
            totalRecords++;
        }
    }
    for (int i = 0; i < count; i++) { dirty[i] = comps[(size_t)i].m_bIsDirty; frameLastChange[i] = comps[(size_t)i].m_frameLastChange; }
    return total;
}

// the LinearDepth render target (device memory owned by the caller), wired as the node's "depthStencil" parameter
RT_API void sailor_rt_set_depth(SailorRuntime* rt, void* devicePtr, int width, int height)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    rt->depth = hip->WrapTexture(devicePtr, { width, height }, EFormat::R32_SFLOAT);
    if (rt->lightCulling) rt->lightCulling->SetRHIResource("depthStencil", rt->depth);
}

// the raw reversed-Z depth attachment (caller's device memory) in front of a "LinearizeDepth" node whose target is the
// LinearDepth render target set with sailor_rt_set_depth (DefaultRenderer.renderer: LinearizeDepth -> LightCulling)
RT_API void sailor_rt_set_raw_depth(SailorRuntime* rt, void* devicePtr, int width, int height)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    rt->rawDepth = hip->WrapTexture(devicePtr, { width, height }, EFormat::R32_SFLOAT);
    if (rt->linearizeDepth) {
        rt->linearizeDepth->SetRHIResource("depthStencil", rt->rawDepth);
        if (rt->depth) rt->linearizeDepth->SetRHIResource("target", rt->depth);
    }
}

RT_API void sailor_rt_set_surface(SailorRuntime* rt, void* surfaceDevicePtr, void* radianceDevicePtr, int width, int height)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    rt->surface = hip->WrapBuffer(surfaceDevicePtr, (size_t)width * height * 48);
    rt->radiance = hip->WrapBuffer(radianceDevicePtr, (size_t)width * height * 16);
    if (rt->renderScene) { rt->renderScene->SetRHIResource("surface", rt->surface); rt->renderScene->SetRHIResource("radiance", rt->radiance); }
}

// The scene RenderScene draws when it has no "surface" resource (RHISceneViewSnapshot::m_batches / m_sceneBindings): one vertex and one index buffer shared by
// the batches (as a mesh pool is), the per-instance, material and texture-descriptor SSBOs (a null pointer leaves that binding out), and the batches as host
// records {indexCount, instanceCount, firstIndex, vertexOffset, firstInstance}.  numBatches = 0 clears the scene.
RT_API int sailor_rt_set_scene(SailorRuntime* rt, void* vertices, uint32_t numVertices, void* indices, uint32_t numIndices, void* instances, uint32_t numInstances,
                               void* materials, uint32_t numMaterials, void* textures, uint32_t numTextures, const uint32_t* batches, int numBatches)
{
    if (!rt || numBatches < 0 || (numBatches > 0 && !batches)) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    rt->snapshot.m_batches.clear();
    rt->snapshot.m_sceneBindings = Renderer::GetDriver()->CreateShaderBindings();
    if (instances) rt->snapshot.m_sceneBindings->GetOrAddShaderBinding("data")->m_buffer = hip->WrapBuffer(instances, (size_t)numInstances * sizeof(SailorPerInstanceData));
    if (materials) rt->snapshot.m_sceneBindings->GetOrAddShaderBinding("material")->m_buffer = hip->WrapBuffer(materials, (size_t)numMaterials * sizeof(SailorMaterialData));
    if (textures) rt->snapshot.m_sceneBindings->GetOrAddShaderBinding("textureSamplers")->m_buffer = hip->WrapBuffer(textures, (size_t)numTextures * sizeof(SailorTextureDesc));
    RHIBufferPtr vb = vertices ? hip->WrapBuffer(vertices, (size_t)numVertices * sizeof(SailorVertexP3N3T3B3UV2C4)) : RHIBufferPtr();
    RHIBufferPtr ib = indices ? hip->WrapBuffer(indices, (size_t)numIndices * 4) : RHIBufferPtr();
    for (int i = 0; i < numBatches; i++) {
        RHISceneBatch b;
        b.m_vertexBuffer = vb; b.m_indexBuffer = ib;
        b.m_indexCount = batches[5 * i]; b.m_instanceCount = batches[5 * i + 1]; b.m_firstIndex = batches[5 * i + 2]; b.m_vertexOffset = batches[5 * i + 3];
        b.m_firstInstance = batches[5 * i + 4];
        rt->snapshot.m_batches.push_back(b);
    }
    return 0;
}

// RHITexture::GetMipLevels() of the textures behind the scene's `textureSamplers` table, one per descriptor, after sailor_rt_set_scene (which forgets them):
// what the engine knows of its textures on the host.  The surface pass takes the entry points with the implicit level of detail iff an entry exceeds 1;
// without this call the route is the one-level one.  -1, and nothing changed, unless n is the table's length.
RT_API int sailor_rt_set_scene_texture_levels(SailorRuntime* rt, const uint32_t* levels, int n)
{
    if (!rt || n < 0 || (n > 0 && !levels) || !rt->snapshot.m_sceneBindings) return -1;
    auto binding = rt->snapshot.m_sceneBindings->Find("textureSamplers");
    if (!binding || !binding->m_buffer || binding->m_buffer->m_size != (size_t)n * sizeof(SailorTextureDesc)) return -1;
    binding->m_buffer->m_hipTextureLevels.assign(levels, levels + n);
    return 0;
}

// IGraphicsDriver::CreateTexture with a full chain + IGraphicsDriverCommands::GenerateMipMaps for one 2-D RGBA8 image, as the TextureImporter does for every
// texture it loads: the whole chain (sailor_hip_mip_chain_texels(width, height, full) texels) back into `outChain`.  -1 on any refusal.
RT_API int sailor_rt_generate_texture_mips(SailorRuntime* rt, const void* rgba8, int width, int height, int srgb, uint32_t* outChain, size_t outTexels)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    const uint32_t full = sailor_hip_texture_mip_levels(width, height);
    if (!rt || !rgba8 || !outChain || !full || outTexels != sailor_hip_mip_chain_texels(width, height, (int32_t)full)) return -1;
    auto texture = hip->CreateTexture(rgba8, (size_t)width * height * 4, ivec2 { width, height }, srgb ? EFormat::R8G8B8A8_SRGB : EFormat::R8G8B8A8_UNORM, full);
    if (!texture || texture->GetMipLevels() != full) return -1;
    auto cmd = hip->CreateCommandList();
    hip->GenerateMipMaps(cmd, texture);
    hip->SubmitCommandList(cmd);
    hip->WaitIdle();
    return sailor_hip_buffer_download(hip->GetContext(), outChain, texture->m_buffer->m_hip.m_devicePtr, 0, outTexels * 4) == SAILOR_HIP_OK ? 0 : -1;
}

// The materials of the batches sailor_rt_set_scene set (call it afterwards; sailor_rt_set_scene itself leaves every batch untagged, without cutout, back faces
// culled): `tags` is the batches' render queue tags in order, separated by commas, an empty field = untagged (scene_tags.h; NULL = all untagged); flags[i] is
// SAILOR_RT_BATCH_ALPHA_CUTOUT | SAILOR_RT_BATCH_DOUBLE_SIDED of batch i.  -1, and nothing changed, unless numBatches is the scene's and both parse.
RT_API int sailor_rt_set_scene_tags(SailorRuntime* rt, const char* tags, const uint32_t* flags, int numBatches)
{
    if (!rt || numBatches < 0 || (size_t)numBatches != rt->snapshot.m_batches.size()) return -1;
    std::vector<std::string> parsed;
    if (!sailor_rt_parse_scene_tags(tags, numBatches, parsed) || !sailor_rt_scene_flags_ok(flags, numBatches)) return -1;
    for (int i = 0; i < numBatches; i++) {
        RHISceneBatch& b = rt->snapshot.m_batches[(size_t)i];
        b.m_tag = parsed[(size_t)i];
        b.m_bAlphaCutout = (flags[i] & SAILOR_RT_BATCH_ALPHA_CUTOUT) != 0;
        b.m_bDoubleSided = (flags[i] & SAILOR_RT_BATCH_DOUBLE_SIDED) != 0;
    }
    return 0;
}

// The shaders of the batches sailor_rt_set_scene set (call it afterwards; sailor_rt_set_scene itself leaves every batch on Standard.shader): shaders[i] is
// SAILOR_RT_SHADER_STANDARD (0) or SAILOR_RT_SHADER_STANDARD_GLTF (1) of batch i -- a glTF batch's material slots are Standard_glTF.shader's MaterialData.
// -1, and nothing changed, unless numBatches is the scene's and every entry is one of the two.
RT_API int sailor_rt_set_scene_shaders(SailorRuntime* rt, const uint32_t* shaders, int numBatches)
{
    if (!rt || numBatches < 0 || (size_t)numBatches != rt->snapshot.m_batches.size() || !sailor_rt_scene_shaders_ok(shaders, numBatches)) return -1;
    for (int i = 0; i < numBatches; i++) rt->snapshot.m_batches[(size_t)i].m_bGltf = shaders[i] == SAILOR_RT_SHADER_STANDARD_GLTF;
    return 0;
}

// RenderState::m_blendMode and m_bEnableZWrite of the batches' materials (ModelImporter.cpp:213-229 for alphaMode BLEND, MaterialImporter.cpp:329-357 for a .mat
// file): blendModes[i] is EBlendMode (0 None, 1 Additive, 2 AlphaBlending, 3 Multiply), zWrite[i] 0 or 1.  -1, and nothing changed, unless numBatches is the
// scene's and every entry is known.
RT_API int sailor_rt_set_scene_blend(SailorRuntime* rt, const uint32_t* blendModes, const uint32_t* zWrite, int numBatches)
{
    if (!rt || numBatches < 0 || (size_t)numBatches != rt->snapshot.m_batches.size() || !sailor_rt_scene_blend_ok(blendModes, zWrite, numBatches)) return -1;
    for (int i = 0; i < numBatches; i++) {
        rt->snapshot.m_batches[(size_t)i].m_blendMode = (EBlendMode)blendModes[i];
        rt->snapshot.m_batches[(size_t)i].m_bZWrite = zWrite[i] != 0;
    }
    return 0;
}

// the layer budget of a transparent pass (default 4); -1, and nothing changed, outside 1 .. 64
RT_API int sailor_rt_set_transparent_layers(SailorRuntime* rt, int layers)
{
    if (!rt || layers < 0) return -1;
    return static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver())->SetTransparentLayers((uint32_t)layers) ? 0 : -1;
}

// the route of a transparent pass: 0 = peeled by primitive order (default), 1 = per-pixel fragment buckets, one rasterisation a pass and (budget + 1) x 8
// bytes a pixel; the frame's bits and the overflow are the same.  -1, and nothing changed, for any other value
RT_API int sailor_rt_set_transparent_mode(SailorRuntime* rt, int mode)
{
    if (!rt) return -1;
    return static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver())->SetTransparentMode(mode) ? 0 : -1;
}

// the overflow of the last frame's transparent pass: the pixels that still had a fragment behind the budget's layers.  A host read that waits for the stream:
// call it at the next frame's start (or after the frame), as sailor_hip_exchange_adapt's status is read; the recorded frame never reads it.  -1 on failure.
RT_API long long sailor_rt_transparent_overflow(SailorRuntime* rt)
{
    if (!rt) return -1;
    uint32_t pixels = 0;
    return static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver())->TransparentOverflow(pixels) == 0 ? (long long)pixels : -1;
}

// RenderScene's attachments for those draws: "color" (RGBA32F, e.g. Main) and "depthStencil" (the raw R32F DepthBuffer of the prepass, or null)
RT_API int sailor_rt_set_scene_targets(SailorRuntime* rt, void* color, void* depth, int width, int height)
{
    if (!rt || (!rt->renderScene && rt->queueNodes.empty()) || !color) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    std::vector<FrameGraphNodePtr> nodes = rt->queueNodes; // every queue's pass renders into the same attachments (DefaultRenderer.renderer: Main, DepthBuffer)
    if (rt->renderScene) nodes.push_back(rt->renderScene);
    auto colorTexture = hip->WrapTexture(color, { width, height }, EFormat::R32G32B32A32_SFLOAT);
    auto depthTexture = depth ? hip->WrapTexture(depth, { width, height }, EFormat::R32_SFLOAT) : RHITexturePtr();
    for (auto& node : nodes) {
        node->SetRHIResource("color", colorTexture);
        if (depthTexture) node->SetRHIResource("depthStencil", depthTexture);
    }
    return 0;
}

RT_API void sailor_rt_set_shadow_maps(SailorRuntime* rt, void* const* mapDevicePtrs, const int* sizes, const int* formats, const float* lightsMatrices64)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    TVector<RHITexturePtr> maps;
    for (int k = 0; k < SAILOR_NUM_CSM_CASCADES; k++) {
        const EFormat f = formats[k] == SAILOR_SHADOWMAP_R16_SFLOAT ? EFormat::R16_SFLOAT : (formats[k] == SAILOR_SHADOWMAP_R32_SFLOAT ? EFormat::R32_SFLOAT : EFormat::R32G32B32A32_SFLOAT);
        maps.push_back(hip->WrapTexture(mapDevicePtrs[k], { sizes[k], sizes[k] }, f));
    }
    rt->lighting->SetShadowMaps(maps, lightsMatrices64);
}

// the image-based-lighting inputs: published to the frame graph the way EnvironmentNode does (SetSampler, EnvironmentNode.cpp:79,169-170),
// the AO target as render target "g_AO" (RHIFrameGraph.cpp:155)
RT_API void sailor_rt_set_ibl(SailorRuntime* rt, void* irradiance, int irrSize, void* env, int envSize, int envLevels, void* lut, int lutW, int lutH,
                              void* ao, int width, int height)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto irr = hip->WrapTexture(irradiance, { irrSize, irrSize * 6 }, EFormat::R32G32B32A32_SFLOAT);
    size_t envTexels = 0;
    for (int l = 0; l < envLevels; l++) { const int s = (envSize >> l) > 1 ? (envSize >> l) : 1; envTexels += (size_t)6 * s * s; }
    auto e = hip->WrapTexture(env, { 1, (int32_t)envTexels }, EFormat::R32G32B32A32_SFLOAT);
    e->m_extent = { envSize, envSize };
    e->m_mipLevels = (uint32_t)envLevels;
    irr->m_extent = { irrSize, irrSize };
    rt->graph.SetSampler("g_irradianceCubemap", irr);
    rt->graph.SetSampler("g_envCubemap", e);
    rt->graph.SetSampler("g_brdfSampler", hip->WrapTexture(lut, { lutW, lutH }, EFormat::R32G32_SFLOAT));
    if (ao) rt->graph.SetRenderTarget("g_AO", hip->WrapTexture(ao, { width, height }, EFormat::R32_SFLOAT));
}

// The raw environment the Environment node bakes from: published as the sampler "g_skyCubemap" the way SkyNode does, and the node is marked dirty
// (SkyNode::MarkDirty -> EnvironmentNode::MarkDirty).  irradianceSize > 0 overrides the node's 32 x 32 x 6 output (a test knob).
RT_API int sailor_rt_set_sky_cubemap(SailorRuntime* rt, void* cubeChain, int size, int levels, int irradianceSize, void* ao, int width, int height)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    if (!rt->environment) return -1;
    rt->graph.SetSampler("g_skyCubemap", hip->WrapCubemap(cubeChain, size, (uint32_t)levels, EFormat::R32G32B32A32_SFLOAT));
    if (irradianceSize > 0) rt->environment->SetFloat("IrradianceMapSize", (float)irradianceSize);
    static_cast<EnvironmentNode*>(rt->environment.GetRawPtr())->MarkDirty();
    if (ao) rt->graph.SetRenderTarget("g_AO", hip->WrapTexture(ao, { width, height }, EFormat::R32_SFLOAT));
    return 0;
}

// The Sky node of the loaded graph: replace its parameters (SkyNode::GetSkyParams) and, with markDirty != 0, restart its cube bake (SkyNode::MarkDirty)
static SkyNode* sky_node(SailorRuntime* rt) { return rt ? static_cast<SkyNode*>(rt->graph.GetGraphNode("Sky").DynamicCast<SkyNode>().GetRawPtr()) : nullptr; }

RT_API int sailor_rt_sky_set_params(SailorRuntime* rt, const SailorSkyParams* params, int markDirty)
{
    auto* sky = sky_node(rt);
    if (!sky || !params) return -1;
    sky->GetSkyParams() = *params;
    if (markDirty) sky->MarkDirty();
    return 0;
}

// The three textures of the cloud march, which the reference's node loads (Textures/CloudsMap.png) or loads-or-generates (CloudsNoiseLow.bin 128^3,
// CloudsNoiseHigh.bin 32^3) itself (SkyNode.cpp:254-339): caller-owned device bytes here -- weather = mapHeight x mapWidth RGBA8, the volumes size^3 R8, x fastest.
// With them published and cloudsDensity > 0 the node draws "Clouds", the sun behind them, "Compose" and "Blit Clouds"; it then needs "g_noiseSampler"
// (sailor_rt_set_sampler) and its `linearDepth` attachment, and a frame without either returns -1 from sailor_rt_process_frame.
RT_API int sailor_rt_sky_set_cloud_textures(SailorRuntime* rt, void* weather, int mapWidth, int mapHeight, void* noiseLow, int lowSize, void* noiseHigh, int highSize)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto* sky = sky_node(rt);
    if (!sky || !weather || !noiseLow || !noiseHigh || mapWidth <= 0 || mapHeight <= 0 || lowSize <= 0 || highSize <= 0) return -1;
    auto map = hip->WrapTexture(weather, { mapWidth, mapHeight }, EFormat::R8G8B8A8_UNORM);
    auto low = hip->WrapTexture(noiseLow, { lowSize, lowSize }, EFormat::R8_UNORM), high = hip->WrapTexture(noiseHigh, { highSize, highSize }, EFormat::R8_UNORM);
    low->m_depth = lowSize; low->m_buffer->m_size = (size_t)lowSize * lowSize * lowSize;
    high->m_depth = highSize; high->m_buffer->m_size = (size_t)highSize * highSize * highSize;
    sky->SetCloudTextures(map, low, high);
    return 0;
}

// The star mesh of the Sky node, which the reference parses from Content/BSC5 itself (SkyNode.cpp:31-113): caller-owned device memory here --
// `vertices` = count x 3 floats of positions and, at the next 16-byte boundary, count x 4 floats of colours (the outputs of sailor_host_sky_star_mesh).  The
// index buffer (index i = i, :90) is created here.  With the mesh published and "Shaders/Stars.shader" enabled the node draws the star points.
RT_API int sailor_rt_sky_set_stars(SailorRuntime* rt, void* vertices, int count)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto* sky = sky_node(rt);
    if (!sky || !hip || !vertices || count <= 0 || count > 65536) return -1;
    const size_t colorsAt = ((size_t)count * 12 + 15) / 16 * 16;
    std::vector<uint32_t> identity((size_t)count);
    for (int i = 0; i < count; i++) identity[(size_t)i] = (uint32_t)i;
    auto indices = hip->CreateBuffer(identity.size() * 4);
    if (!indices || sailor_hip_buffer_upload(hip->GetContext(), indices->m_hip.m_devicePtr, 0, identity.data(), identity.size() * 4) != SAILOR_HIP_OK) return -1;
    sky->SetStars(hip->WrapBuffer(vertices, colorsAt + (size_t)count * 16), indices, (uint32_t)count);
    return 0;
}

// What the ExperimentalParticles node's loaders read themselves (ParticlesNode.cpp:35-52: Particle_2.yaml's header and the .dat records; :89-101: the first mesh
// of Particle.gltf), published in one call: the header fields, `records` = numRecords x SailorParticleData on the HOST (the node uploads them once, :156), the mesh
// as caller-owned device memory (SailorVertexP3N3T3B3UV2C4 vertices, uint32 indices).  mapWidth x mapHeight is the extent of the node's shadow map (4096 x 4096 in
// the reference, :66), materialInstance what the material's `material` binding would have given the instances (:148).  0, or -1 without such a node in the graph.
RT_API int sailor_rt_set_particles(SailorRuntime* rt, uint32_t n, uint32_t frames, uint32_t fps, uint32_t traceFrames, float traceDecay, const void* records,
                                   uint32_t numRecords, void* vertices, uint32_t numVertices, void* indices, uint32_t numIndices, uint32_t materialInstance, int mapWidth,
                                   int mapHeight)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto* node = rt ? static_cast<ParticlesNode*>(rt->graph.GetGraphNode("ExperimentalParticles").DynamicCast<ParticlesNode>().GetRawPtr()) : nullptr;
    if (!node || !hip || !records || numRecords < n || !vertices || !indices || numVertices == 0 || numIndices < 3 || mapWidth <= 0 || mapHeight <= 0) return -1;
    ParticlesNode::Header header;
    header.m_n = n; header.m_frames = frames; header.m_fps = fps; header.m_traceFrames = traceFrames; header.m_traceDecay = traceDecay;
    const auto* first = static_cast<const SailorParticleData*>(records);
    node->SetShadowMapExtent({ mapWidth, mapHeight });
    node->SetParticles(header, std::vector<SailorParticleData>(first, first + numRecords), hip->WrapBuffer(vertices, (size_t)numVertices * sizeof(SailorVertexP3N3T3B3UV2C4)),
                       hip->WrapBuffer(indices, (size_t)numIndices * 4), numIndices, materialInstance);
    return 0;
}

// the node's instance SSBO and its shadow map once a frame has created them (device pointers; NULL before)
RT_API int sailor_rt_particles_buffers(SailorRuntime* rt, void** outInstances, uint32_t* outNumInstances, void** outShadowMap, int* outWidth, int* outHeight)
{
    auto* node = rt ? static_cast<ParticlesNode*>(rt->graph.GetGraphNode("ExperimentalParticles").DynamicCast<ParticlesNode>().GetRawPtr()) : nullptr;
    if (!node) return -1;
    auto instances = node->GetInstances();
    auto map = node->GetShadowMap();
    if (outInstances) *outInstances = instances ? instances->m_hip.m_devicePtr : nullptr;
    if (outNumInstances) *outNumInstances = instances ? (uint32_t)(instances->m_size / sizeof(SailorParticleInstance)) : 0;
    if (outShadowMap) *outShadowMap = map && map->m_buffer ? map->m_buffer->m_hip.m_devicePtr : nullptr;
    if (outWidth) *outWidth = map ? map->GetExtent().x : 0;
    if (outHeight) *outHeight = map ? map->GetExtent().y : 0;
    return 0;
}

// m_updateEnvCubemapPattern and m_bIsDirty of the Sky node (SkyNode.h:173-174)
RT_API int sailor_rt_sky_state(SailorRuntime* rt, int* outPattern, int* outDirty)
{
    auto* sky = sky_node(rt);
    if (!sky) return -1;
    if (outPattern) *outPattern = (int)sky->GetUpdateEnvCubemapPattern();
    if (outDirty) *outDirty = sky->IsDirty() ? 1 : 0;
    return 0;
}

// The other source of the raw environment: an equirect panorama (the node's "EnvironmentMap" texture, EnvironmentNode.cpp:100-138).  The harness
// hands over the loaded RGBA32F texture; the node converts it to a 512 x 512 x 6 cube with 10 mips and bakes from that.
RT_API int sailor_rt_set_environment_map(SailorRuntime* rt, void* equirect, int width, int height, int repeat, int irradianceSize)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    if (!rt->environment || !equirect) return -1;
    auto tex = hip->WrapTexture(equirect, { width, height }, EFormat::R32G32B32A32_SFLOAT);
    tex->m_bRepeat = repeat != 0;
    if (irradianceSize > 0) rt->environment->SetFloat("IrradianceMapSize", (float)irradianceSize);
    static_cast<EnvironmentNode*>(rt->environment.GetRawPtr())->SetEnvironmentMap(tex);
    return 0;
}

// A file texture the `.renderer` text names under `samplers:` (g_noiseSampler: Textures/Noise.png), which the parser records and does not load:
// the caller hands over the decoded linear RGBA32F texels and the graph publishes them under the sampler's name (RHIFrameGraph::SetSampler,
// what FrameGraphParser.cpp:133-149 does once the TextureImporter has loaded the file).
RT_API int sailor_rt_set_sampler(SailorRuntime* rt, const char* name, void* texels, int width, int height)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    if (!rt || !name || !texels || width <= 0 || height <= 0) return -1;
    rt->graph.SetSampler(name, hip->WrapTexture(texels, { width, height }, EFormat::R32G32B32A32_SFLOAT));
    return 0;
}

// device pointer + geometry of a sampler the graph's nodes published (g_brdfSampler, g_envCubemap, g_irradianceCubemap, ...)
RT_API void* sailor_rt_sampler(SailorRuntime* rt, const char* name, int* outWidth, int* outHeight, int* outLevels)
{
    auto t = rt->graph.GetSampler(name);
    if (!t || !t->m_buffer) return nullptr;
    if (outWidth) *outWidth = t->GetExtent().x;
    if (outHeight) *outHeight = t->GetExtent().y;
    if (outLevels) *outLevels = (int)t->GetMipLevels();
    return t->m_buffer->m_hip.m_devicePtr;
}

// The blur section of ShadowPrepassNode::Process (FrameGraph/ShadowPrepassNode.cpp:283-356) for one EVSM cascade, command for command: the
// radius upload (:286), "Blur Horizontal" (shadow map -> temporary target) and "Blur Vertical" (temporary target -> shadow map).  (The caster draws
// in front of it need a rasteriser and are not part of this path.)
RT_API int sailor_rt_blur_shadow_map(SailorRuntime* rt, void* mapDevicePtr, void* tempDevicePtr, int size, float radiusUmbra, float radiusPenumbra)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    auto shadowMap = hip->WrapTexture(mapDevicePtr, { size, size }, EFormat::R32G32B32A32_SFLOAT);
    auto blurAttachment = hip->WrapTexture(tempDevicePtr, { size, size }, EFormat::R32G32B32A32_SFLOAT); // GetOrAddTemporaryRenderTarget (:285)
    auto vertical = driver->CreateMaterial(driver->CreateShader("Shaders/Blur.shader", { "VERTICAL", "EVSM" }));     // :60-62
    auto horizontal = driver->CreateMaterial(driver->CreateShader("Shaders/Blur.shader", { "HORIZONTAL", "EVSM" })); // :65-67
    auto blurBindings = driver->CreateShaderBindings();                                                             // :70
    auto blurData = driver->AddBufferToShaderBindings(blurBindings, "data", 48, 0, EShaderBindingType::UniformBuffer); // :73 (3 x vec4)
    auto frameBindings = driver->CreateShaderBindings();
    auto cmd = driver->CreateCommandList();
    const float blurRadius[2] = { radiusUmbra, radiusPenumbra };
    if (radiusUmbra * radiusUmbra + radiusPenumbra * radiusPenumbra > 0.01f) { // m_blurRadius.length() > 0.1f (:283)
        commands->UpdateShaderBinding(cmd, blurData, blurRadius, sizeof blurRadius); // :286
        commands->BeginDebugRegion(cmd, "Blur Horizontal");
        driver->AddSamplerToShaderBindings(blurBindings, "colorSampler", shadowMap, 1); // :292
        commands->ImageMemoryBarrier(cmd, shadowMap, EImageLayout::ShaderReadOnlyOptimal);
        commands->ImageMemoryBarrier(cmd, blurAttachment, EImageLayout::ColorAttachmentOptimal);
        commands->BeginRenderPass(cmd, TVector<RHITexturePtr> { blurAttachment }, RHITexturePtr());
        commands->BindMaterial(cmd, horizontal);
        commands->BindShaderBindings(cmd, horizontal, { frameBindings, blurBindings });
        commands->DrawIndexed(cmd, 6, 1, 0, 0, 0);
        commands->EndRenderPass(cmd);
        commands->EndDebugRegion(cmd);
        commands->BeginDebugRegion(cmd, "Blur Vertical");
        driver->AddSamplerToShaderBindings(blurBindings, "colorSampler", blurAttachment, 1); // :329
        commands->BeginRenderPass(cmd, TVector<RHITexturePtr> { shadowMap }, RHITexturePtr());
        commands->BindMaterial(cmd, vertical);
        commands->BindShaderBindings(cmd, vertical, { frameBindings, blurBindings });
        commands->DrawIndexed(cmd, 6, 1, 0, 0, 0);
        commands->EndRenderPass(cmd);
        commands->EndDebugRegion(cmd);
    }
    driver->SubmitCommandList(cmd);
    return hip->GetLastDispatchStatus();
}

// The "GPU Culling" section of RHIRecordDrawCallGPUCulling (RHI/Batch.hpp:146-188) over resident buffers: the indirect buffer is bound as
// "drawIndexedIndirect" (:86-89), the push constants are { numBatches, numInstances, firstInstanceIndex } (:176-184) and the Dispatch binds
// { computeMeshCullingBindings (depthHighZ), perInstanceData, indirect buffer, frame } (RenderSceneNode.cpp:335).  The frame UBO is the one
// RHIFrameGraph::FillFrameData uploads for the current camera / viewport.
RT_API int sailor_rt_gpu_culling(SailorRuntime* rt, void* instancesDevicePtr, uint32_t numInstances, uint32_t firstInstanceIndex, void* batchesDevicePtr,
                                 uint32_t numBatches)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    auto transferCmdList = driver->CreateCommandList();
    rt->graph.FillFrameData(transferCmdList, rt->snapshot, rt->snapshot.m_deltaTime, rt->snapshot.m_currentTime);
    // RenderSceneNode.cpp:126-139: the shader is loaded with its OCCLUSION_CULLING define and the node's "depthHighZ" attachment is bound as a sampler
    // (here: when sailor_rt_build_depth_highz has produced a pyramid; otherwise the frustum-only build)
    auto computeCullingShader = rt->depthHighZ ? driver->CreateShader("Shaders/ComputeMeshCulling.shader", { "OCCLUSION_CULLING" })
                                               : driver->CreateShader("Shaders/ComputeMeshCulling.shader");
    auto computeMeshCullingBindings = driver->CreateShaderBindings();
    if (rt->depthHighZ) driver->AddSamplerToShaderBindings(computeMeshCullingBindings, "depthHighZ", rt->depthHighZ, 0);
    auto perInstanceData = driver->CreateShaderBindings();
    perInstanceData->GetOrAddShaderBinding("data")->m_buffer = hip->WrapBuffer(instancesDevicePtr, (size_t)(firstInstanceIndex + numInstances) * sizeof(SailorPerInstanceData));
    auto indirectCommandBufferBinding = driver->CreateShaderBindings();
    if (batchesDevicePtr)
        indirectCommandBufferBinding->GetOrAddShaderBinding("drawIndexedIndirect")->m_buffer = hip->WrapBuffer(batchesDevicePtr, (size_t)numBatches * sizeof(SailorDrawIndexedIndirectData));
    struct PushConstants { uint32_t m_numBatches = 0, m_numInstances = 0, m_firstInstanceIndex = 0; } constants;
    constants.m_numBatches = numBatches;
    constants.m_numInstances = numInstances;
    constants.m_firstInstanceIndex = firstInstanceIndex;
    commands->BeginDebugRegion(transferCmdList, "GPU Culling");
    commands->Dispatch(transferCmdList, computeCullingShader, 256, 1, 1,
                       { computeMeshCullingBindings, perInstanceData, indirectCommandBufferBinding, rt->snapshot.m_frameBindings }, &constants, sizeof constants);
    commands->EndDebugRegion(transferCmdList);
    driver->SubmitCommandList(transferCmdList);
    return hip->GetLastDispatchStatus();
}

// The indirect buffer of node `nodeIndex` of the graph (a DepthPrepass node, or a RenderScene node under `GPUCulling: true`) after its last frame, downloaded
// (this waits for the device): up to maxCommands records of 5 words into `out`.  Returns the number of commands the node wrote, -1 for any other node and
// before the node's first frame.
static void* node_indirect_buffer(SailorRuntime* rt, int nodeIndex, int* outCommands)
{
    if (!rt || nodeIndex < 0 || (size_t)nodeIndex >= rt->graph.GetGraph().size()) return nullptr;
    const auto& node = rt->graph.GetGraph()[(size_t)nodeIndex];
    const SceneIndirectDraws* draws = nullptr;
    if (auto prepass = node.DynamicCast<DepthPrepassNode>()) draws = &prepass->GetIndirectDraws();
    else if (auto scene = node.DynamicCast<RenderSceneNode>()) draws = &scene->GetIndirectDraws();
    if (!draws || !draws->GetIndirectBuffer()) return nullptr;
    if (outCommands) *outCommands = (int)draws->GetNumCommands();
    return draws->GetIndirectBuffer()->m_hip.m_devicePtr;
}
RT_API int sailor_rt_node_indirect_commands(SailorRuntime* rt, int nodeIndex, uint32_t* out, int maxCommands)
{
    int count = 0;
    void* device = node_indirect_buffer(rt, nodeIndex, &count);
    if (!device) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    hip->WaitIdle();
    const int n = count < maxCommands ? count : maxCommands;
    if (out && n > 0 && sailor_hip_buffer_download(hip->GetContext(), out, device, 0, (size_t)n * sizeof(SailorDrawIndexedIndirectData)) != SAILOR_HIP_OK) return -1;
    return count;
}

// The debug regions of the last sailor_rt_process_frame in the order the driver EXECUTED their BeginDebugRegion commands while it submitted the frame's lists
// (HipGraphicsDriver::GetExecutedRegions), joined by ';'.  Returns their number.
RT_API int sailor_rt_last_frame_regions(SailorRuntime* rt, char* out, int outSize)
{
    if (!rt) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    std::string s;
    for (const auto& r : hip->GetExecutedRegions()) s += (s.empty() ? "" : ";") + r;
    if (out && outSize > 0) snprintf(out, (size_t)outSize, "%s", s.c_str());
    return (int)hip->GetExecutedRegions().size();
}

// One depth-only pass of one DrawIndexedIndirect over batch 0 of the scene with a material of `shaderPath`, recorded and submitted at once: what a node would
// record with that material.  Returns the driver's status afterwards (it stays the status sailor_rt_process_frame returns): 0 for a routed shader,
// SAILOR_HIP_ERR_UNSUPPORTED for any other.
RT_API int sailor_rt_draw_indexed_indirect(SailorRuntime* rt, const char* shaderPath, void* depthDevicePtr, int width, int height)
{
    if (!rt || !shaderPath || !depthDevicePtr || rt->snapshot.m_batches.empty()) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    auto cmd = driver->CreateCommandList();
    rt->graph.FillFrameData(cmd, rt->snapshot, rt->snapshot.m_deltaTime, rt->snapshot.m_currentTime);
    const RHISceneBatch& b = rt->snapshot.m_batches[0];
    SailorDrawIndexedIndirectData data {};
    data.indexCount = b.m_indexCount; data.instanceCount = b.m_instanceCount; data.firstIndex = b.m_firstIndex; data.vertexOffset = (int32_t)b.m_vertexOffset;
    data.firstInstance = b.m_firstInstance;
    auto indirect = driver->CreateIndirectBuffer(sizeof data);
    if (!indirect) return -1;
    commands->UpdateBuffer(cmd, indirect, &data, sizeof data, 0);
    auto material = driver->CreateMaterial(driver->CreateShader(shaderPath));
    commands->BeginRenderPass(cmd, TVector<RHITexturePtr> {}, hip->WrapTexture(depthDevicePtr, { width, height }, EFormat::R32_SFLOAT), true);
    commands->BindMaterial(cmd, material);
    commands->BindShaderBindings(cmd, material, { rt->snapshot.m_frameBindings, rt->snapshot.m_sceneBindings });
    commands->BindVertexBuffer(cmd, b.m_vertexBuffer, 0);
    commands->BindIndexBuffer(cmd, b.m_indexBuffer, 0);
    commands->DrawIndexedIndirect(cmd, indirect, 0, 1, sizeof data);
    commands->EndRenderPass(cmd);
    driver->SubmitCommandList(cmd);
    driver->WaitIdle(); // (the indirect buffer is released with this scope)
    return hip->GetLastDispatchStatus();
}

// DefaultRenderer.renderer's DepthHighZ target (R32_SFLOAT, mips, reduction Min) + one run of the DepthHighZ node over a wrapped depth image.
// The pyramid stays bound for the following sailor_rt_gpu_culling calls; levels <= 0 drops it again.
RT_API int sailor_rt_build_depth_highz(SailorRuntime* rt, void* depthDevicePtr, int depthWidth, int depthHeight, int width, int height, int levels, void** outPyramid)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto driver = Renderer::GetDriver();
    if (levels <= 0) { rt->depthHighZ.Clear(); return 0; }
    auto node = FrameGraphBuilder::CreateNode("DepthHighZ");
    if (!node) return -1;
    rt->depthHighZ = driver->CreateRenderTarget({ width, height }, (uint32_t)levels, EFormat::R32_SFLOAT);
    if (!rt->depthHighZ) return -1;
    node->SetRHIResource("src", hip->WrapTexture(depthDevicePtr, { depthWidth, depthHeight }, EFormat::R32_SFLOAT));
    node->SetRHIResource("dst", rt->depthHighZ);
    auto cmd = driver->CreateCommandList();
    node->Process(&rt->graph, cmd, cmd, rt->snapshot);
    driver->SubmitCommandList(cmd);
    node->Clear();
    if (outPyramid) *outPyramid = rt->depthHighZ->m_buffer->m_hip.m_devicePtr;
    return hip->GetLastDispatchStatus();
}

// One shadow pass of ShadowPrepassNode::Process (FrameGraph/ShadowPrepassNode.cpp:219-365), command for command: barriers, BeginRenderPass(shadow map, temporary
// depth attachment, clear), the light matrix as push constant (:249), the caster draw (vertex / index buffer, per-instance SSBO `data`, instanced DrawIndexed --
// what RHIRecordDrawCall records per batch), EndRenderPass, then for an EVSM pass with a blur radius the two blur draws (:283-356).
RT_API int sailor_rt_shadow_pass(SailorRuntime* rt, const float* lightMatrix, void* positions, uint32_t numVertices, void* indices, uint32_t numIndices, void* models,
                                 uint32_t firstInstance, uint32_t instanceCount, void* shadowMapDevicePtr, int size, int evsm, float radiusUmbra, float radiusPenumbra)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    auto shadowMap = hip->WrapTexture(shadowMapDevicePtr, { size, size }, evsm ? EFormat::R32G32B32A32_SFLOAT : EFormat::R16_SFLOAT);
    auto depthAttachment = driver->CreateRenderTarget({ size, size }, 1, EFormat::R32_SFLOAT); // GetOrAddTemporaryRenderTarget(depth format, extent) (:229)
    auto material = evsm ? driver->CreateMaterial(driver->CreateShader("Shaders/ShadowCaster.shader", { "EVSM" }))
                         : driver->CreateMaterial(driver->CreateShader("Shaders/ShadowCaster.shader")); // GetOrAddShadowMaterial (:20-45)
    auto perInstanceData = driver->CreateShaderBindings();
    perInstanceData->GetOrAddShaderBinding("data")->m_buffer = hip->WrapBuffer(models, (size_t)(firstInstance + instanceCount) * 64);
    auto cmd = driver->CreateCommandList();
    commands->BeginDebugRegion(cmd, "Record Shadow Map Pass 0");
    commands->ImageMemoryBarrier(cmd, shadowMap, EImageLayout::ColorAttachmentOptimal);
    commands->ImageMemoryBarrier(cmd, depthAttachment, EImageLayout::General);
    commands->BeginRenderPass(cmd, TVector<RHITexturePtr> { shadowMap }, depthAttachment);
    commands->PushConstants(cmd, material, 64, lightMatrix);
    commands->BindMaterial(cmd, material);
    commands->BindShaderBindings(cmd, material, { rt->snapshot.m_frameBindings ? rt->snapshot.m_frameBindings : driver->CreateShaderBindings(), perInstanceData });
    commands->BindVertexBuffer(cmd, hip->WrapBuffer(positions, (size_t)numVertices * 12), 0);
    commands->BindIndexBuffer(cmd, hip->WrapBuffer(indices, (size_t)numIndices * 4), 0);
    commands->DrawIndexed(cmd, numIndices, instanceCount, 0, 0, firstInstance);
    commands->EndRenderPass(cmd);
    commands->EndDebugRegion(cmd);
    driver->SubmitCommandList(cmd);
    int st = hip->GetLastDispatchStatus();
    if (st == 0 && evsm && radiusUmbra * radiusUmbra + radiusPenumbra * radiusPenumbra > 0.01f) {
        auto temp = driver->CreateRenderTarget({ size, size }, 1, EFormat::R32G32B32A32_SFLOAT);
        st = sailor_rt_blur_shadow_map(rt, shadowMapDevicePtr, temp->m_buffer->m_hip.m_devicePtr, size, radiusUmbra, radiusPenumbra);
        driver->WaitIdle(); // `temp` is released on return
    }
    return st;
}

// split frame: this runtime renders tile-row band `rank` of `worldSize` (targets set afterwards hold the band's rows); `comm` = ncclComm_t or null
RT_API int sailor_rt_set_frame_split(SailorRuntime* rt, int rank, int worldSize, void* comm)
{
    (void)rt;
    return static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver())->SetFrameSplit(rank, worldSize, comm);
}

// the RCCL step: the band lists of the last frame -> the reference's global buffers, in caller-owned device memory
RT_API int sailor_rt_exchange_light_lists(SailorRuntime* rt, void* globalGridDevicePtr, size_t gridBytes, void* globalCulledDevicePtr, size_t culledBytes)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto node = rt->lightCulling.DynamicCast<LightCullingNode>();
    if (!node || !node->GetCulledLights()) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    auto g = node->GetCulledLights()->Find("lightsGrid"), c = node->GetCulledLights()->Find("culledLights");
    if (!g || !c || !g->m_buffer || !c->m_buffer) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    return hip->ExchangeLightLists(g->m_buffer, c->m_buffer, hip->WrapBuffer(globalGridDevicePtr, gridBytes), hip->WrapBuffer(globalCulledDevicePtr, culledBytes));
}

// a wrapped RGBA32F device image as a named render target of the graph (the HDR target RenderScene's radiance stands for, an LDR target of the caller's)
RT_API void sailor_rt_set_color_target(SailorRuntime* rt, const char* name, void* devicePtr, int width, int height)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    rt->graph.SetRenderTarget(name, hip->WrapTexture(devicePtr, { width, height }, EFormat::R32G32B32A32_SFLOAT));
}

// the same with a mip chain behind level 0 (`Main`, DefaultRenderer.renderer:24-31): devicePtr is a level-major RGBA32F chain of sailor_hip_mip_chain_texels(
// width, height, levels) texels whose head -- level 0 -- may be the very buffer RenderScene writes its radiance to
RT_API int sailor_rt_set_color_target_chain(SailorRuntime* rt, const char* name, void* devicePtr, int width, int height, int levels)
{
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    if (!rt || !name || !devicePtr || levels < 1 || sailor_hip_mip_chain_texels(width, height, levels) == 0) return -1;
    rt->graph.SetRenderTarget(name, hip->WrapRenderTarget(devicePtr, { width, height }, (uint32_t)levels, EFormat::R32G32B32A32_SFLOAT));
    return 0;
}

// sceneView.m_deltaTime / m_currentTime of the frames processed from here on (EyeAdaptationNode.cpp:162 reads the first)
RT_API void sailor_rt_set_time(SailorRuntime* rt, float deltaTime, float currentTime)
{
    rt->snapshot.m_deltaTime = deltaTime;
    rt->snapshot.m_currentTime = currentTime;
}

// the EyeAdaptation node's state, for read-back: the device pointers of its `histogram` SSBO (256 uint32) and of its 1 x 1 average-luminance target (one float)
RT_API int sailor_rt_eye_adaptation_state(SailorRuntime* rt, void** outHistogram, void** outLuminance)
{
    for (const auto& n : rt->graph.GetGraph()) {
        auto node = n.DynamicCast<EyeAdaptationNode>();
        if (!node) continue;
        auto lum = node->GetAverageLuminance();
        auto hist = node->GetHistogramBindings() ? node->GetHistogramBindings()->Find("histogram") : RHIShaderBindingPtr();
        if (!lum || !lum->m_buffer || !hist || !hist->m_buffer) return -1;
        if (outHistogram) *outHistogram = hist->m_buffer->m_hip.m_devicePtr;
        if (outLuminance) *outLuminance = lum->m_buffer->m_hip.m_devicePtr;
        return 0;
    }
    return -1;
}

// ---- the world's DebugContext (RHI/DebugContext.h): what game code calls through World::GetDebugContext(); the DebugDraw node draws what it holds ----------------
RT_API int sailor_rt_debug_draw_line(SailorRuntime* rt, const float* start3, const float* end3, const float* color4, float duration)
{
    if (!rt || !start3 || !end3 || !color4) return -1;
    rt->debug.DrawLine(start3, end3, color4, duration);
    return 0;
}
RT_API int sailor_rt_debug_draw_aabb(SailorRuntime* rt, const float* min3, const float* max3, const float* color4, float duration)
{
    if (!rt || !min3 || !max3 || !color4) return -1;
    rt->debug.DrawAABB(min3, max3, color4, duration);
    return 0;
}
RT_API int sailor_rt_debug_draw_frustum(SailorRuntime* rt, const float* corners24, const float* color4, float duration)
{
    if (!rt || !corners24 || !color4) return -1;
    rt->debug.DrawFrustum(corners24, color4, duration);
    return 0;
}
RT_API int sailor_rt_debug_draw_origin(SailorRuntime* rt, const float* position3, const float* origin16, float size, float duration)
{
    if (!rt || !position3 || !origin16) return -1;
    rt->debug.DrawOrigin(position3, origin16, size, duration);
    return 0;
}
RT_API int sailor_rt_debug_draw_sphere(SailorRuntime* rt, const float* position3, float radius, const float* color4, float duration)
{
    if (!rt || !position3 || !color4) return -1;
    rt->debug.DrawSphere(position3, radius, color4, duration);
    return 0;
}
RT_API int sailor_rt_debug_draw_arrow(SailorRuntime* rt, const float* start3, const float* end3, const float* color4, float duration)
{
    if (!rt || !start3 || !end3 || !color4) return -1;
    rt->debug.DrawArrow(start3, end3, color4, duration);
    return 0;
}
// DebugContext::Tick(transferCmd, deltaTime) as the world's tick calls it before the frame is rendered: upload, then the lifetimes.  Returns the number of
// vertices the next frame draws (m_numRenderedVertices), -1 without a runtime.
RT_API int sailor_rt_debug_tick(SailorRuntime* rt, float deltaTime)
{
    if (!rt) return -1;
    auto transferCmd = Renderer::GetDriver()->CreateCommandList();
    rt->debug.Tick(transferCmd, deltaTime);
    Renderer::GetDriver()->SubmitCommandList(transferCmd);
    return (int)rt->debug.GetNumRenderedVertices();
}
// the line list as it stands (after the last tick's expiry): up to maxVertices VertexP3C4 records into outVertices (may be null); returns the vertex count
RT_API int sailor_rt_debug_vertices(SailorRuntime* rt, float* outVertices, int maxVertices)
{
    if (!rt) return -1;
    const auto& v = rt->debug.GetLineVertices();
    if (outVertices)
        for (size_t i = 0; i < v.size() && (int)i < maxVertices; i++) memcpy(outVertices + 7 * i, &v[i], sizeof(SailorVertexP3C4));
    return (int)v.size();
}

// ---- the frame's ImGui draw data (Submodules/ImGuiApi.cpp): what ImGui::Render() left, as plain arrays -- per list its buffer sizes and its run of commands,
// the lists' vertex and 16-bit index buffers one behind the other.  Mirrors ImGui_Init (:295-332: the material of ImGuiUI.shader -- TriangleList,
// AlphaBlending --, the RGBA8 font atlas as `sTexture`; done at the first call and whenever a font is given) and ImGui_UpdateDrawData (:129-188: create or
// grow the frame's vertex and index buffer, upload every list).  numLists == 0 or a null vertex pointer takes the draw data away.  Returns the number of
// commands that will draw, -1 on a bad argument.
RT_API int sailor_rt_set_ui_draw_data(SailorRuntime* rt, const float* displayPos2, const float* displaySize2, const float* framebufferScale2, const void* vertices,
                                      uint32_t numVertices, const uint16_t* indices, uint32_t numIndices, const SailorUiDrawList* lists, uint32_t numLists,
                                      const SailorUiDrawCmd* cmds, uint32_t numCmds, const void* fontRgba8, int fontWidth, int fontHeight)
{
    if (!rt) return -1;
    if (!vertices || !numLists) { rt->snapshot.m_drawImGui = nullptr; return 0; }
    if (!displayPos2 || !displaySize2 || !framebufferScale2 || !indices || !lists || (numCmds && !cmds) || !numVertices || !numIndices) return -1;
    uint64_t vtx = 0, idx = 0;
    for (uint32_t n = 0; n < numLists; n++) {
        if ((uint64_t)lists[n].firstCmd + lists[n].cmdCount > numCmds) return -1;
        vtx += lists[n].vtxCount; idx += lists[n].idxCount;
    }
    if (vtx != numVertices || idx != numIndices) return -1; // the lists' buffers are exactly what was handed over
    auto* driver = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    auto commands = Renderer::GetDriverCommands();
    RHIImGuiDrawData& ui = rt->ui;
    if (!ui.m_material) { // ImGui_Init
        auto shader = driver->CreateShader("Shaders/ImGuiUI.shader");
        if (!shader || !shader->IsReady()) return -1;
        ui.m_material = driver->CreateMaterial(shader);
        ui.m_material->m_blendMode = EBlendMode::AlphaBlending;
        ui.m_material->m_topology = EPrimitiveTopology::TriangleList;
        ui.m_material->m_bDoubleSided = true; // ECullMode::None
    }
    if (fontRgba8 && fontWidth > 0 && fontHeight > 0) {
        auto font = driver->CreateTexture(fontRgba8, (size_t)fontWidth * fontHeight * 4, ivec2 { fontWidth, fontHeight }, EFormat::R8G8B8A8_UNORM);
        if (!font) return -1;
        ui.m_shaderBindings = driver->CreateShaderBindings();
        driver->AddSamplerToShaderBindings(ui.m_shaderBindings, "sTexture", font, 0);
    }
    if (!ui.m_shaderBindings) ui.m_shaderBindings = driver->CreateShaderBindings(); // no atlas yet: `sTexture` unbound, which samples as 0
    for (int k = 0; k < 2; k++) { ui.m_displayPos[k] = displayPos2[k]; ui.m_displaySize[k] = displaySize2[k]; ui.m_framebufferScale[k] = framebufferScale2[k]; }
    ui.m_vertices.assign((const VertexP2UV2C1*)vertices, (const VertexP2UV2C1*)vertices + numVertices);
    ui.m_indices.assign(indices, indices + numIndices);
    ui.m_lists.assign(lists, lists + numLists);
    ui.m_cmds.assign(cmds, cmds + numCmds);
    // ImGui_UpdateDrawData
    const size_t vertexSize = ui.m_vertices.size() * sizeof(VertexP2UV2C1), indexSize = ui.m_indices.size() * sizeof(uint16_t);
    if (!ui.m_vertexBuffer || ui.m_vertexBuffer->m_size < vertexSize) ui.m_vertexBuffer = driver->CreateBuffer(vertexSize);
    if (!ui.m_indexBuffer || ui.m_indexBuffer->m_size < indexSize) ui.m_indexBuffer = driver->CreateBuffer((indexSize + 3) / 4 * 4);
    if (!ui.m_vertexBuffer || !ui.m_indexBuffer) return -1;
    auto transferCmd = driver->CreateCommandList();
    size_t vOffset = 0, iOffset = 0;
    for (uint32_t n = 0; n < numLists; n++) { // (:173-185)
        const size_t vSize = lists[n].vtxCount * sizeof(VertexP2UV2C1), iSize = lists[n].idxCount * sizeof(uint16_t);
        if (vSize) commands->UpdateBuffer(transferCmd, ui.m_vertexBuffer, (const char*)ui.m_vertices.data() + vOffset, vSize, vOffset);
        if (iSize) commands->UpdateBuffer(transferCmd, ui.m_indexBuffer, (const char*)ui.m_indices.data() + iOffset, iSize, iOffset);
        vOffset += vSize; iOffset += iSize;
    }
    driver->SubmitCommandList(transferCmd);
    // what will draw, and a workspace for it: grown here, outside the frame's recorded commands
    float pc[4];
    uint32_t count = 0;
    if (sailor_host_ui_flatten(ui.m_displayPos, ui.m_displaySize, ui.m_framebufferScale, ui.m_lists.data(), numLists, ui.m_cmds.data(), numCmds, pc, nullptr, 0, &count, nullptr,
                               nullptr) != SAILOR_HIP_OK)
        return -1;
    uint64_t triangles = 0;
    for (auto& c : ui.m_cmds) triangles += c.elemCount / 3u;
    if (!driver->ReserveUiWorkspace((uint32_t)std::min<uint64_t>(triangles, 0xFFFFFFFFull))) return -1;
    rt->snapshot.m_drawImGui = &rt->ui;
    return (int)count;
}

// ---- the cascades: what LightingECS::PrepareCSMPasses reads of the scene, and what it decided ------------------------------------------------------------
// The scene's caster data, after sailor_rt_set_scene: the world boxes of the scene's instances on the device (numInstances x SailorAABB, what
// sailor_hip_ecs_sweep writes), m_bCastShadows as a host bitmask (NULL = every instance casts), the frame each instance last changed (host, one per instance),
// the cascade maps' resolutions (4 ints, NULL = ECS/LightingECS.h:67) and how the overlap sets are traced (SAILOR_TRACE_*; ~0u = as the runtime's sweep
// system does, flat without one; rootSize 0 = the reference's).  From then on every sailor_rt_process_frame runs FillLightingData's shadow half first and
// a ShadowPrepass node draws what it asks for.  A null box pointer takes the caster data away again.
RT_API int sailor_rt_set_caster_data(SailorRuntime* rt, void* worldAabbDevicePtr, uint32_t numInstances, const uint64_t* castShadows, const uint64_t* lastChangedFrames,
                                     const int* resolutions, uint32_t traceMode, uint32_t rootSize)
{
    if (!rt) return -1;
    if (!worldAabbDevicePtr) { rt->lighting->SetCasterData(nullptr); rt->snapshot.m_shadowMapsToUpdate.clear(); return 0; }
    if (numInstances && !lastChangedFrames) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    CsmCasterData casters;
    casters.m_worldAabb = hip->WrapBuffer(worldAabbDevicePtr, (size_t)numInstances * sizeof(SailorAABB));
    casters.m_numInstances = numInstances;
    const size_t words = ((size_t)numInstances + 63) / 64;
    if (castShadows) casters.m_castShadows.assign(castShadows, castShadows + words);
    casters.m_lastChangedFrame.assign(lastChangedFrames, lastChangedFrames + numInstances);
    for (int k = 0; resolutions && k < SAILOR_NUM_CSM_CASCADES; k++) {
        if (resolutions[k] <= 0) return -1;
        casters.m_resolutions[k] = { resolutions[k], resolutions[k] };
    }
    if (traceMode == ~0u) { casters.m_traceMode = rt->sweep ? rt->sweep->GetTraceMode() : SAILOR_TRACE_FLAT_FLOAT_BOXES; casters.m_rootSize = rt->sweep ? rt->sweep->GetRootSize() : 0u; }
    else if (traceMode == SAILOR_TRACE_FLAT_FLOAT_BOXES || traceMode == SAILOR_TRACE_OCTREE_INT_BOXES) { casters.m_traceMode = traceMode; casters.m_rootSize = rootSize; }
    else return -1;
    rt->lighting->SetCasterData(&casters);
    return 0;
}

// the owner's rotation of one light (x, y, z, w): with its position the light's transform, whose inverse is RHILightProxy::m_lightMatrix (LightingECS.cpp:227)
RT_API int sailor_rt_set_light_rotation(SailorRuntime* rt, int index, const float* rotation4)
{
    if (!rt || !rotation4 || index < 0 || (size_t)index >= rt->lighting->Num()) return -1;
    memcpy(rt->lighting->GetComponentData((size_t)index).m_ownerRotation, rotation4, 16);
    return 0;
}

// sceneView.m_shadowMapsToUpdate of the last frame: per pass 8 words {m_lighMatrixIndex, m_shadowType, casters, dependencies, up to three dependency indices, 0};
// outMasks (may be null): the passes' caster masks, `wordsPerMask` words each.  Returns the number of passes.
RT_API int sailor_rt_shadow_passes(SailorRuntime* rt, uint32_t* outInfo, uint64_t* outMasks, uint32_t wordsPerMask, int maxPasses)
{
    if (!rt) return -1;
    const auto& passes = rt->snapshot.m_shadowMapsToUpdate;
    for (int i = 0; i < (int)passes.size() && i < maxPasses; i++) {
        const auto& p = passes[(size_t)i];
        if (outInfo) {
            uint32_t* o = outInfo + 8 * i;
            o[0] = p.m_lighMatrixIndex; o[1] = (uint32_t)p.m_shadowType; o[2] = p.m_numCasters; o[3] = (uint32_t)p.m_internalCommandsList.size();
            for (int k = 0; k < 3; k++) o[4 + k] = k < (int)p.m_internalCommandsList.size() ? p.m_internalCommandsList[(size_t)k] : 0u;
            o[7] = 0;
        }
        if (outMasks)
            for (uint32_t w = 0; w < wordsPerMask; w++) outMasks[(size_t)i * wordsPerMask + w] = w < p.m_casterMask.size() ? p.m_casterMask[w] : 0ull;
    }
    return (int)passes.size();
}

// cascade map k of the runtime's LightingECS (m_csmShadowMaps, LightingECS.cpp:53-63): device pointer, size and SAILOR_SHADOWMAP_* format; null before the first
// frame with caster data
RT_API void* sailor_rt_csm_shadow_map(SailorRuntime* rt, int cascade, int* outSize, int* outFormat)
{
    if (!rt || cascade < 0 || (size_t)cascade >= rt->lighting->GetCsmShadowMaps().size()) return nullptr;
    const auto& map = rt->lighting->GetCsmShadowMaps()[(size_t)cascade];
    if (outSize) *outSize = map->GetExtent().x;
    if (outFormat) *outFormat = map->m_format == EFormat::R16_SFLOAT ? SAILOR_SHADOWMAP_R16_SFLOAT : SAILOR_SHADOWMAP_R32G32B32A32_SFLOAT;
    return map->m_buffer->m_hip.m_devicePtr;
}

// `lightsMatrices` of the lights set as the frames recorded so far left it: 4 x mat4 (a uniform block on this backend: its bytes live on the host)
RT_API int sailor_rt_lights_matrices(SailorRuntime* rt, float* out64)
{
    auto b = rt && rt->lighting->GetLightsData() ? rt->lighting->GetLightsData()->Find("lightsMatrices") : RHIShaderBindingPtr();
    if (!b || b->m_hostCopy.size() < 256 || !out64) return -1;
    memcpy(out64, b->m_hostCopy.data(), 256);
    return 0;
}

// LightingECS's pass planning without a renderer (no device needed): the host half of PrepareCSMPasses (LightingECS::PlanLightPasses) and the batches' runs
// (LightingECS::CountBatchRuns) over overlap sets the caller supplies, with m_csmSnapshots carried from frame to frame by the planner.
struct SailorCsmPlanner { SailorCsmSnapshots* snapshots = nullptr; };
RT_API SailorCsmPlanner* sailor_rt_csm_planner_create() { return new SailorCsmPlanner(); }
RT_API void sailor_rt_csm_planner_destroy(SailorCsmPlanner* planner)
{
    if (planner) sailor_host_csm_snapshots_destroy(planner->snapshots);
    delete planner;
}
// One frame: numLights directional lights in component order (their shadow types, their SailorCsmView of this frame), overlapMasks = numLights x 4 x
// ceil(numInstances / 64) words, batchRanges = numBatches x (firstInstance, instanceCount).  Per pass: outInfo 8 words {light, m_lighMatrixIndex, m_shadowType,
// casters, dependencies, up to three dependency indices}, outMasks ceil(numInstances / 64) words, outRuns numBatches x (count, offset).  Returns the number of
// passes (the first maxPasses are written), -1 on a bad argument.
RT_API int sailor_rt_csm_planner_frame(SailorCsmPlanner* planner, uint32_t numLights, const uint32_t* lightShadowTypes, const SailorCsmView* views, uint32_t numInstances,
                                       const uint64_t* overlapMasks, const uint64_t* lastChangedFrame, const uint64_t* castShadows, const uint32_t* batchRanges,
                                       uint32_t numBatches, uint32_t maxPasses, uint32_t* outInfo, uint64_t* outMasks, uint32_t* outRuns)
{
    if (!planner || (numLights && (!lightShadowTypes || !views || !overlapMasks)) || (numInstances && !lastChangedFrame) || (numBatches && !batchRanges)) return -1;
    const uint32_t numCsmSnapshots = numLights * LightingECS::NumCascades; // ECS/LightingECS.cpp:391-397
    if (planner->snapshots && sailor_host_csm_snapshots_count(planner->snapshots) != numCsmSnapshots) { sailor_host_csm_snapshots_destroy(planner->snapshots); planner->snapshots = nullptr; }
    if (!planner->snapshots) planner->snapshots = sailor_host_csm_snapshots_create();
    if (!planner->snapshots) return -1;
    const size_t words = ((size_t)numInstances + 63) / 64;
    TVector<RHISceneBatch> batches(numBatches);
    for (uint32_t b = 0; b < numBatches; b++) { batches[b].m_firstInstance = batchRanges[2 * b]; batches[b].m_instanceCount = batchRanges[2 * b + 1]; }
    uint32_t placed = 0;
    for (uint32_t light = 0; light < numLights; light++) {
        const auto plans = LightingECS::PlanLightPasses(planner->snapshots, light * LightingECS::NumCascades, placed, numInstances,
                                                        overlapMasks + (size_t)light * LightingECS::NumCascades * words, (EShadowType)lightShadowTypes[light],
                                                        lastChangedFrame, views + light, castShadows);
        for (const CsmPassPlan& plan : plans) {
            if (placed < maxPasses) {
                TVector<RHIShadowBatchRun> runs;
                const uint32_t casters = LightingECS::CountBatchRuns(plan.m_casterMask, batches, runs);
                if (outInfo) {
                    uint32_t* o = outInfo + 8 * (size_t)placed;
                    o[0] = light; o[1] = plan.m_cascade; o[2] = (uint32_t)plan.m_shadowType; o[3] = casters; o[4] = (uint32_t)plan.m_internalCommandsList.size();
                    for (int k = 0; k < 3; k++) o[5 + k] = k < (int)plan.m_internalCommandsList.size() ? plan.m_internalCommandsList[(size_t)k] : 0u;
                }
                if (outMasks) memcpy(outMasks + (size_t)placed * words, plan.m_casterMask.data(), words * 8);
                if (outRuns)
                    for (uint32_t b = 0; b < numBatches; b++) { outRuns[((size_t)placed * numBatches + b) * 2] = runs[b].m_count; outRuns[((size_t)placed * numBatches + b) * 2 + 1] = runs[b].m_offset; }
            }
            placed++;
        }
    }
    return (int)placed;
}

// ---- frame capture (a test facility, off by default): see the frame between its entries -------------------------------------------------------------------
// A named resource as it is bound right now: a device range, or host bytes (a uniform block), or neither (absent).  Names: a render target or a published
// sampler / cube of the graph (its whole buffer: every mip level, every face), "lightsGrid" / "culledLights" (the LightCulling node's SSBOs), "light" (the
// lights SSBO), "lightsMatrices" (a host block on this backend), "csm0" .. "csm3" (the cascade maps), "eyeAdaptation" (the EyeAdaptation node's state: 256
// counts and the adapted luminance), "indirect<i>" (the indirect commands of graph node i, 20 bytes each).
static GraphicsDriver::HIP::HipGraphicsDriver::CaptureCopy capture_source(SailorRuntime* rt, const std::string& name)
{
    GraphicsDriver::HIP::HipGraphicsDriver::CaptureCopy c;
    auto of_buffer = [&c](const RHIBufferPtr& b) { if (b && b->m_hip.m_devicePtr) { c.m_device = b->m_hip.m_devicePtr; c.m_bytes = b->m_size; } };
    if (name == "lightsGrid" || name == "culledLights") {
        auto node = rt->lightCulling.DynamicCast<LightCullingNode>();
        auto b = node && node->GetCulledLights() ? node->GetCulledLights()->Find(name) : RHIShaderBindingPtr();
        if (b) of_buffer(b->m_buffer);
    } else if (name == "light" || name == "lightsMatrices") {
        auto b = rt->lighting->GetLightsData() ? rt->lighting->GetLightsData()->Find(name) : RHIShaderBindingPtr();
        if (b && b->m_buffer) of_buffer(b->m_buffer);
        else if (b && !b->m_hostCopy.empty()) { c.m_host = b->m_hostCopy; c.m_bytes = c.m_host.size(); }
    } else if (name.size() == 4 && name.rfind("csm", 0) == 0 && name[3] >= '0' && name[3] < '0' + SAILOR_NUM_CSM_CASCADES) {
        const size_t k = (size_t)(name[3] - '0');
        if (k < rt->lighting->GetCsmShadowMaps().size() && rt->lighting->GetCsmShadowMaps()[k]) of_buffer(rt->lighting->GetCsmShadowMaps()[k]->m_buffer);
    } else if (name == "eyeAdaptation") {
        for (const auto& n : rt->graph.GetGraph()) {
            auto node = n.DynamicCast<EyeAdaptationNode>();
            auto hist = node && node->GetHistogramBindings() ? node->GetHistogramBindings()->Find("histogram") : RHIShaderBindingPtr();
            if (hist) { of_buffer(hist->m_buffer); break; }
        }
    } else if (name.rfind("indirect", 0) == 0 && name.size() > 8 && name.find_first_not_of("0123456789", 8) == std::string::npos) {
        int commands = 0;
        if (void* device = node_indirect_buffer(rt, atoi(name.c_str() + 8), &commands)) { c.m_device = device; c.m_bytes = (size_t)commands * sizeof(SailorDrawIndexedIndirectData); }
    } else {
        auto t = rt->graph.GetRenderTarget(name);
        if (!t) t = rt->graph.GetSampler(name);
        if (t) of_buffer(t->m_buffer);
    }
    return c;
}

// Arms a capture of the NEXT sailor_rt_process_frame: `names` (comma-separated, `count` of them) are resolved while that frame is recorded -- before the
// transfer list (slot 0), before the first entry (slot 1: the whole transfer list has executed by then, which is where the nodes' transfer-list work shows)
// and after each graph node i (slot 2 + i) -- and their bytes copied, in that place of the frame, to storage + slot * sum(capacities) + the capacities before
// it.  A resource that does not exist at a slot (a cube before the frame that creates it) is absent there, not an error; one larger than its capacity is not
// copied and reported.  Returns the number of slots (nodes + 2); -1 on a bad argument or too little storage; the unsupported status while the driver's stream
// is being captured into a hipGraph.  Nothing is recorded, and nothing differs, in a frame that was not armed.
RT_API int sailor_rt_capture_next_frame(SailorRuntime* rt, const char* names, const size_t* capacities, int count, void* storage, size_t storageBytes)
{
    if (!rt || !names || !capacities || count <= 0 || !storage) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    if (hip->IsStreamCapturing() != 0) return SAILOR_HIP_ERR_UNSUPPORTED; // fails closed: a stream whose capture status cannot be read is refused too
    std::vector<std::string> list;
    for (const char* p = names;;) {
        const char* e = strchr(p, ',');
        list.emplace_back(p, e ? (size_t)(e - p) : strlen(p));
        if (!e) break;
        p = e + 1;
    }
    if ((int)list.size() != count) return -1;
    std::vector<size_t> offsets((size_t)count);
    size_t stride = 0;
    for (int k = 0; k < count; k++) { offsets[(size_t)k] = stride; stride += capacities[k]; }
    const int slots = (int)rt->graph.GetGraph().size() + RHIFrameGraph::CaptureSlotFirstNode;
    if (stride == 0 || storageBytes / stride < (size_t)slots) return -1;
    std::vector<size_t> caps(capacities, capacities + count);
    rt->captureSlots = slots;
    rt->captureBytes.assign((size_t)slots * count, -1);
    rt->graph.CaptureNextFrame([rt, hip, list, offsets, caps, stride, storage, slots](RHICommandListPtr cmd, int slot) {
        if (slot < 0 || slot >= slots) return;
        TVector<GraphicsDriver::HIP::HipGraphicsDriver::CaptureCopy> copies;
        for (size_t k = 0; k < list.size(); k++) {
            auto c = capture_source(rt, list[k]);
            long long& bytes = rt->captureBytes[(size_t)slot * list.size() + k];
            if (!c.m_device && c.m_host.empty()) { bytes = -1; continue; }
            if (c.m_bytes > caps[k]) { bytes = -2; continue; }
            bytes = (long long)c.m_bytes;
            c.m_offset = (size_t)slot * stride + offsets[k];
            copies.push_back(std::move(c));
        }
        hip->RecordCapture(cmd, storage, std::move(copies));
    });
    return slots;
}

// what the last armed frame recorded: [slot][name] = bytes copied, -1 absent, -2 larger than its capacity; returns slots x names (0 before any capture)
RT_API int sailor_rt_capture_result(SailorRuntime* rt, long long* out, int maxEntries)
{
    if (!rt) return -1;
    for (int i = 0; out && i < (int)rt->captureBytes.size() && i < maxEntries; i++) out[i] = rt->captureBytes[(size_t)i];
    return (int)rt->captureBytes.size();
}

RT_API int sailor_rt_process_frame(SailorRuntime* rt)
{
    static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver())->ClearExecutedRegions();
    if (rt->lighting->HasCasterData()) { // FillLightingData's shadow half (ECS/LightingECS.cpp:377-401): the world's tick runs it before the frame is rendered
        const int st = rt->lighting->FillShadowPasses(rt->snapshot);
        if (st != SAILOR_HIP_OK) return st;
    }
    rt->graph.Process(rt->snapshot);
    rt->frames++;
    return static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver())->GetLastDispatchStatus();
}

// One frame in which ANOTHER command overwrites the cull's two SSBOs between the LightCulling node and RenderScene (what a debug pass or a host-side
// list editor would record): the shade must read what the write leaves there -- on a split frame too, where the band form's tile blocks and split
// blocks must decide "long tile" on the same bytes.  gridData / culledData: host bytes for lightsGrid / culledLights (either may be null).
RT_API int sailor_rt_process_frame_overwriting_lists(SailorRuntime* rt, const void* gridData, size_t gridBytes, const void* culledData, size_t culledBytes)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    auto node = rt->lightCulling.DynamicCast<LightCullingNode>();
    if (!node) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (rt->lighting->HasCasterData()) { // as sailor_rt_process_frame: this frame's shadow passes, not the last one's
        const int st = rt->lighting->FillShadowPasses(rt->snapshot);
        if (st != SAILOR_HIP_OK) return st;
    }
    auto transferCmdList = driver->CreateCommandList();
    auto cmdList = driver->CreateCommandList();
    rt->graph.FillFrameData(transferCmdList, rt->snapshot, rt->snapshot.m_deltaTime, rt->snapshot.m_currentTime);
    for (auto& n : rt->graph.GetGraph()) n->Prepare(&rt->graph, rt->snapshot);
    for (auto& n : rt->graph.GetGraph()) {
        n->Process(&rt->graph, transferCmdList, cmdList, rt->snapshot);
        if (n.GetRawPtr() != rt->lightCulling.GetRawPtr() || !node->GetCulledLights()) continue;
        auto g = node->GetCulledLights()->Find("lightsGrid"), c = node->GetCulledLights()->Find("culledLights");
        if (gridData && g && g->m_buffer && gridBytes <= g->m_buffer->m_size) commands->UpdateBuffer(cmdList, g->m_buffer, gridData, gridBytes, 0);
        if (culledData && c && c->m_buffer && culledBytes <= c->m_buffer->m_size) commands->UpdateBuffer(cmdList, c->m_buffer, culledData, culledBytes, 0);
    }
    driver->SubmitCommandList(transferCmdList);
    driver->SubmitCommandList(cmdList);
    rt->frames++;
    return static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(driver)->GetLastDispatchStatus();
}

// the launch log of the driver's context (sailor_hip_context_launch_log): how many kernels the frames recorded so far, and the names of the last few --
// what lets a test say that a node recorded nothing
RT_API int sailor_rt_launch_log(SailorRuntime* rt, uint64_t* outCount, const char** outNames, int maxNames)
{
    if (!rt) return -1;
    auto* hip = static_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    return hip ? sailor_hip_context_launch_log(hip->GetContext(), outCount, outNames, maxNames) : -1;
}

RT_API void sailor_rt_wait_idle(SailorRuntime*) { Renderer::GetDriver()->WaitIdle(); }

// device pointers of the node-owned SSBOs, for read-back by the tests
RT_API void* sailor_rt_buffer(SailorRuntime* rt, const char* name, size_t* outBytes)
{
    if (name && !strcmp(name, "light")) { // LightingECS's `light` SSBO (LightingECS.cpp:44)
        auto lb = rt->lighting->GetLightsData()->Find("light");
        if (!lb || !lb->m_buffer) return nullptr;
        if (outBytes) *outBytes = lb->m_buffer->m_size;
        return lb->m_buffer->m_hip.m_devicePtr;
    }
    auto node = rt->lightCulling.DynamicCast<LightCullingNode>();
    if (!node || !node->GetCulledLights()) return nullptr;
    auto b = node->GetCulledLights()->Find(name);
    if (!b || !b->m_buffer) return nullptr;
    if (outBytes) *outBytes = b->m_buffer->m_size;
    return b->m_buffer->m_hip.m_devicePtr;
}

RT_API int sailor_rt_ecs_sweep(SailorRuntime* rt, const void* transforms, const uint32_t* parent, const void* localAabb, uint32_t count,
                               const uint32_t* levelOffsets, uint32_t numLevels, void** outWorld, void** outWorldAabb, void** outVisibility)
{
    rt->sweep.reset(new EcsSweepSystem((const SailorTransform*)transforms, parent, (const SailorAABB*)localAabb, count, levelOffsets, numLevels));
    const auto& c = rt->snapshot.m_camera;
    const int st = rt->sweep->Tick(c.m_world, c.m_aspect, c.m_fov, c.m_zNear, c.m_zFar);
    *outWorld = rt->sweep->m_world->m_hip.m_devicePtr;
    *outWorldAabb = rt->sweep->m_worldAabb->m_hip.m_devicePtr;
    *outVisibility = rt->sweep->m_visibility->m_hip.m_devicePtr;
    return st;
}

// the same with EcsSweepSystem's trace mode set first (SAILOR_TRACE_*, rootSize 0 = the reference's); *outInserted = the inserted words (octree mode) or NULL
RT_API int sailor_rt_ecs_sweep_traced(SailorRuntime* rt, const void* transforms, const uint32_t* parent, const void* localAabb, uint32_t count,
                                      const uint32_t* levelOffsets, uint32_t numLevels, uint32_t mode, uint32_t rootSize, void** outWorld,
                                      void** outWorldAabb, void** outVisibility, void** outInserted)
{
    rt->sweep.reset(new EcsSweepSystem((const SailorTransform*)transforms, parent, (const SailorAABB*)localAabb, count, levelOffsets, numLevels));
    rt->sweep->SetTraceMode(mode, rootSize);
    const auto& c = rt->snapshot.m_camera;
    const int st = rt->sweep->Tick(c.m_world, c.m_aspect, c.m_fov, c.m_zNear, c.m_zFar);
    *outWorld = rt->sweep->m_world->m_hip.m_devicePtr;
    *outWorldAabb = rt->sweep->m_worldAabb->m_hip.m_devicePtr;
    *outVisibility = rt->sweep->m_visibility->m_hip.m_devicePtr;
    *outInserted = rt->sweep->m_inserted ? rt->sweep->m_inserted->m_hip.m_devicePtr : nullptr;
    return st;
}
