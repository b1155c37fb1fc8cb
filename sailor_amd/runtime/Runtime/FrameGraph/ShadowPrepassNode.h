// Mirrors Runtime/FrameGraph/ShadowPrepassNode.{h,cpp}: the node that draws the cascades LightingECS::PrepareCSMPasses asked for
// (sceneView.m_shadowMapsToUpdate) -- per pass the caster draws into the cascade's map over a temporary depth attachment, the draws of the passes it
// depends on, the pass's light matrix into `lightsMatrices`, and for an EVSM pass the two blur draws.
// In the reference this is a TFrameGraphNode<ShadowPrepassNode> and registers under "ShadowPrepass"; here the class derives from the base directly and is
// created by FrameGraphBuilder::CreateOptInNode for graphs that enabled it, like BloomNode (FrameGraphNode.h says why: older tests use the name as their
// example of an entry without a node class).
#pragma once
#include "FrameGraphNode.h"

namespace Sailor::Framegraph {

class ShadowPrepassNode : public BaseFrameGraphNode {
public:
    struct PerInstanceData { float model[16]; }; // ShadowPrepassNode.h: { mat4 model; }, the record of ShadowCaster.shader's PerInstanceDataSSBO
    static const char* GetName() { return m_name; }
    std::string GetDebugName() const override { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    RHI::RHIMaterialPtr GetOrAddShadowMaterial(RHI::EShadowType shadowType); // ShadowPrepassNode.cpp:20-45 (one vertex description on this path)
    static const char* m_name;
    RHI::RHIMaterialPtr m_shadowMaterial_Pcf, m_shadowMaterial_Evsm;
    RHI::RHIShaderPtr m_pBlurVerticalShader, m_pBlurHorizontalShader;
    RHI::RHIMaterialPtr m_pBlurVerticalMaterial, m_pBlurHorizontalMaterial;
    RHI::RHIShaderBindingSetPtr m_pBlurShaderBindings;
    RHI::RHIShaderBindingPtr m_lightMatrices;
    RHI::RHIShaderBindingSetPtr m_perInstanceData; // `data`: every pass's matrices, pass after pass
    size_t m_sizePerInstanceData = 0;
    // what the mirror keeps beside them: the passes' bitmasks on the device (the gather's input), and per vertex buffer of the view its vec3 positions
    // (ShadowCaster.shader's vertex input; extracted when the view first hands that buffer over, dropped when it no longer does)
    RHI::RHIBufferPtr m_masks;
    TVector<std::pair<RHI::RHIBufferPtr, RHI::RHIBufferPtr>> m_positions; // (the view's vertex buffer, its positions)
};

} // namespace Sailor::Framegraph
