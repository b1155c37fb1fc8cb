// Mirrors Runtime/FrameGraph/DepthPrepassNode.h / .cpp:50-303.  Its draws are recorded as RenderSceneNode's are under `GPUCulling` (SceneIndirectDraws.h).
#pragma once
#include "FrameGraphNode.h"
#include "SceneIndirectDraws.h"

namespace Sailor::Framegraph {

// `DepthPrepass` of DefaultRenderer.renderer: `Tag` (the render queue: a batch is drawn if its own tag is empty or equal), `ClearDepth`, `GPUCulling`,
// "depthStencil" and optionally "depthHighZ".  The depth material is Shaders/DepthOnly.shader; a batch that requires a custom depth shader (ALPHA_CUTOUT: a
// `Masked` batch) is its own depth material with the define and its five binding sets (DepthPrepassNode.cpp:246-255) -- here { frame, lights, scene }.
// BeginRenderPass({}, depthStencil, clear) has no colour attachment: the backend ends the pass with the depth write alone.
class DepthPrepassNode : public TFrameGraphNode<DepthPrepassNode> {
public:
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;
    const SceneIndirectDraws& GetIndirectDraws() const { return m_draws; }

protected:
    static const char* m_name;
    RHI::RHIShaderPtr m_pDepthShader, m_pCutoutShaders[2];  // DepthOnly; Standard / Standard_glTF with ALPHA_CUTOUT
    RHI::RHIMaterialPtr m_pDepthMaterials[2];               // [double-sided]
    RHI::RHIMaterialPtr m_pCutoutMaterials[4];              // [glTF * 2 + double-sided]
    SceneIndirectDraws m_draws;
};

} // namespace Sailor::Framegraph
