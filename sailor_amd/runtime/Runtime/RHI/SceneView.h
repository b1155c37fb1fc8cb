// Mirrors RHI/SceneView.h:60-83 RHISceneViewSnapshot -- the per-camera snapshot handed to every node's Process.
#pragma once
#include "Types.h"

namespace Sailor::RHI {

struct CameraData { // ECS/CameraECS.h: what the nodes read from sceneView.m_camera
    float m_world[16];
    float m_fov = 90.0f, m_aspect = 1.0f, m_zNear = 1.0f, m_zFar = 20000.0f;
};

// One batch of RHISceneViewProxy / RHIRecordDrawCall (RHI/Batch.hpp) as RenderSceneNode.cpp draws it: a mesh's buffers and the arguments of its DrawIndexed
struct RHISceneBatch {
    RHIBufferPtr m_vertexBuffer, m_indexBuffer; // VertexP3N3T3B3UV2C4 records; uint32 indices
    uint32_t m_indexCount = 0, m_instanceCount = 0, m_firstIndex = 0, m_vertexOffset = 0, m_firstInstance = 0;
    // the batch's material, as far as RenderSceneNode.cpp and the backend need it (AssetRegistry/Model/ModelImporter.cpp:213-229): its render queue tag
    // ("Opaque", "Masked"; empty = drawn by every RenderScene node, as before the tags existed), ALPHA_CUTOUT (alphaMode == "MASK") and the cull mode
    // (doubleSided = ECullMode::None).  The defaults are the batch of before: untagged, no cutout, back faces culled.
    std::string m_tag;
    bool m_bAlphaCutout = false;
    bool m_bDoubleSided = false;
    // the batch's shader is Shaders/Standard_glTF.shader, what ModelImporter.cpp:156-231 gives every imported model, and its material slots are that shader's
    // MaterialData; false = Shaders/Standard.shader
    bool m_bGltf = false;
    // RenderState::m_bEnableZWrite and m_blendMode of the batch's material: a glTF material with alphaMode == "BLEND" has the render queue Transparent, z-write
    // off and blend None (ModelImporter.cpp:213-229); a .mat file chooses its blendMode (MaterialImporter.cpp:329-357).  The defaults are the batch of before.
    bool m_bZWrite = true;
    EBlendMode m_blendMode = EBlendMode::None;
};

enum class EShadowType : uint32_t { None = 0, PCF = 1, EVSM = 2 }; // RHI/SceneView.h:13-18

// RHI/SceneView.h:56-65 RHIUpdateShadowMapCommand: one shadow pass of ShadowPrepassNode::Process, as LightingECS::PrepareCSMPasses hands it over.  In place of
// m_meshList (a vector of proxies) the pass carries its caster set as a bitmask over the scene's instances (`data` of m_sceneBindings), LSB first -- the
// cascade's overlap set without what an earlier re-rendered cascade of the same type overlaps (ECS/LightingECS.cpp:305-332), ANDed with m_bCastShadows
// (the node's own filter, ShadowPrepassNode.cpp:110, applied where the mask is made) -- and what the host derives from the mask by popcount: per batch of
// the view, how many of the batch's instances the pass draws and where their run of matrices begins inside the pass's slice of the node's SSBO.
struct RHIShadowBatchRun { uint32_t m_count = 0, m_offset = 0; };
struct RHIUpdateShadowMapCommand {
    uint32_t m_lighMatrixIndex = 0;
    EShadowType m_shadowType = EShadowType::None;
    float m_blurRadius[2] = { 0.0f, 0.0f }; // [Umbra, Penumbra]
    RHITexturePtr m_shadowMap;
    float m_lightMatrix[16] = {};
    TVector<uint32_t> m_internalCommandsList;
    TVector<uint64_t> m_casterMask;         // ceil(instances / 64) words
    TVector<RHIShadowBatchRun> m_batchRuns; // one per entry of RHISceneViewSnapshot::m_batches
    uint32_t m_numCasters = 0;              // the sum of the runs' counts
};

struct RHISceneViewSnapshot {
    CameraData m_camera;
    float m_deltaTime = 0.0f, m_currentTime = 0.0f;
    uint32_t m_totalNumLights = 0;           // RHI/SceneView.h:75, filled at ECS/LightingECS.cpp:404
    RHIShaderBindingSetPtr m_frameBindings;  // :78, filled by RHIFrameGraph::FillFrameData
    RHIShaderBindingSetPtr m_rhiLightsData;  // :79, LightingECS::m_lightsData (binding 0 `light`, 6 `lightsMatrices`, 8 `shadowMaps`)
    TVector<RHIUpdateShadowMapCommand> m_shadowMapsToUpdate; // :76, filled by LightingECS::FillShadowPasses (ECS/LightingECS.cpp:399-400) when the view has caster data
    // what RenderSceneNode.cpp draws: the batches of the view, and Standard.shader's sets 2-4 as one set -- `data` (PerInstanceDataSSBO), `material`
    // (MaterialDataSSBO), `textureSamplers` (a device table of SailorTextureDesc)
    TVector<RHISceneBatch> m_batches;
    RHIShaderBindingSetPtr m_sceneBindings;
    // :81 m_debugDrawSecondaryCmdList is a secondary command list the world's DebugContext recorded DrawDebugMesh into; secondary lists are not mirrored, so
    // the snapshot carries the context itself and DebugDrawNode records its draw directly (null = no debug drawing)
    const class DebugContext* m_debugContext = nullptr;
    // :82 m_drawImGui is the task that records ImGuiApi::ImGui_RenderDrawData into a secondary command list; here the finished frame's draw data itself, as
    // plain arrays, with what ImGuiApi's backend data holds for it (null = no UI this frame).  RenderImGuiNode records its draws directly.
    const struct RHIImGuiDrawData* m_drawImGui = nullptr;
};

// ImDrawData (DisplayPos, DisplaySize, FramebufferScale, the lists' merged buffers as ImGui_UpdateDrawData :170-185 uploads them, the commands) and
// ImGuiApi::Data: the material of ImGui_Init (:295-332), its shader bindings with the font atlas as `sTexture`, the frame's vertex and index buffer
struct RHIImGuiDrawData {
    float m_displayPos[2] = { 0, 0 }, m_displaySize[2] = { 0, 0 }, m_framebufferScale[2] = { 1, 1 };
    TVector<VertexP2UV2C1> m_vertices;      // every list's VtxBuffer, in list order
    TVector<uint16_t> m_indices;            // every list's IdxBuffer (sizeof(ImDrawIdx) == 2)
    TVector<SailorUiDrawList> m_lists;      // per list: its buffer sizes and its run of commands
    TVector<SailorUiDrawCmd> m_cmds;        // per command: ClipRect, ElemCount, IdxOffset, VtxOffset, the callback kind
    RHIMaterialPtr m_material;
    RHIShaderBindingSetPtr m_shaderBindings;
    RHIBufferPtr m_vertexBuffer, m_indexBuffer;
};

} // namespace Sailor::RHI
