// Mirrors Runtime/FrameGraph/ClearNode.{h,cpp}: clears its `target` -- a depth format with ClearDepthStencil(clearDepth, clearStencil), any other with
// ClearImage(clearColor) (DefaultRenderer.renderer:70-84: DepthBuffer to 0 / 0, Main to its clear colour).
// In the reference this is a TFrameGraphNode<ClearNode> and registers under "Clear"; here the class derives from the base directly and is created by
// FrameGraphBuilder::CreateOptInNode for graphs that enabled it, like BloomNode (FrameGraphNode.h says why: older tests use the name as their example of an
// entry without a node class).
#pragma once
#include "FrameGraphNode.h"

namespace Sailor::Framegraph {

class ClearNode : public BaseFrameGraphNode {
public:
    static const char* GetName() { return m_name; }
    std::string GetDebugName() const override { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    static const char* m_name;
};

} // namespace Sailor::Framegraph
