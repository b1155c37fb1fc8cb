// Mirrors the parts of Runtime/FrameGraph/RHIFrameGraph.{h,cpp} the path needs: the ordered node list, named render
// targets, FillFrameData (RHIFrameGraph.cpp:50-73) and the per-frame node walk (RHIFrameGraph.cpp:95,250-252).  The Vulkan-
// specific barrier balancing (:201-246) and command-list chaining (:254-322) are out of scope.
#pragma once
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "BaseFrameGraphNode.h"
#include "../RHI/GraphicsDriver.h"

namespace Sailor::Framegraph {

class RHIFrameGraph {
public:
    void AddNode(FrameGraphNodePtr node) { m_graph.push_back(node); }
    const std::vector<FrameGraphNodePtr>& GetGraph() const { return m_graph; }
    FrameGraphNodePtr GetGraphNode(const std::string& tag) const // RHIFrameGraph.cpp GetGraphNode: the first node with that name
    {
        for (const auto& node : m_graph) if (node->GetDebugName() == tag) return node;
        return FrameGraphNodePtr();
    }
    void SetRenderTarget(const std::string& name, RHI::RHITexturePtr rt) { m_renderTargets[name] = rt; }
    RHI::RHITexturePtr GetRenderTarget(const std::string& name) const
    {
        auto it = m_renderTargets.find(name);
        return it == m_renderTargets.end() ? RHI::RHITexturePtr() : it->second;
    }
    // named samplers published by nodes (EnvironmentNode.cpp:79,169-170 SetSampler("g_brdfSampler" / "g_envCubemap" / "g_irradianceCubemap"))
    void SetSampler(const std::string& name, RHI::RHITexturePtr tex) { m_samplers[name] = tex; }
    RHI::RHITexturePtr GetSampler(const std::string& name) const
    {
        auto it = m_samplers.find(name);
        return it == m_samplers.end() ? RHI::RHITexturePtr() : it->second;
    }
    void SetValue(const std::string& name, float v) { m_values[name] = v; } // RHIFrameGraph.h SetValue (FrameGraphParser.cpp:130)
    float GetValue(const std::string& name, float fallback = 0.0f) const { auto it = m_values.find(name); return it == m_values.end() ? fallback : it->second; }
    // opt-in node classes (FrameGraphBuilder::CreateOptInNode): kept across Clear(), so that it can be set before a `.renderer` text is loaded
    void EnableNode(const std::string& name) { m_enabledNodes.insert(name); }
    bool IsNodeEnabled(const std::string& name) const { return m_enabledNodes.count(name) != 0; }
    void SetViewport(int32_t width, int32_t height) { m_viewport = { width, height }; } // App::GetMainWindow()->GetRenderArea()
    RHI::ivec2 GetViewport() const { return m_viewport; }

    // RHIFrameGraph.cpp:50-72: `frameData` (set 0, binding 0) and `previousFrameData` (binding 1: what MotionBlur.shader:38-48 reads) of the scene view's
    // frame bindings; returns the frame data it uploaded.  The four-argument form passes m_prevFrameData, as RHIFrameGraph.cpp:189 does.
    RHI::UboFrameData FillFrameData(RHI::RHICommandListPtr transferCmdList, RHI::RHISceneViewSnapshot& snapshot, const RHI::UboFrameData& previousFrame, float deltaTime,
                                    float worldTime) const;
    RHI::UboFrameData FillFrameData(RHI::RHICommandListPtr transferCmdList, RHI::RHISceneViewSnapshot& snapshot, float deltaTime, float worldTime) const
    {
        return FillFrameData(transferCmdList, snapshot, m_prevFrameData, deltaTime, worldTime);
    }
    // One frame: FillFrameData, then node->Process in graph order, then submit (record-then-submit)
    void Process(RHI::RHISceneViewSnapshot& snapshot);
    // Frame capture (a test facility, off by default): the hook is called while the NEXT Process() records, then dropped -- with the transfer list and
    // CaptureSlotFrameStart before anything is recorded, with the main list and CaptureSlotBeforeNodes before node 0 (when it executes, the whole transfer
    // list has: the work the nodes record there lies between these two slots), and with the main list and CaptureSlotFirstNode + i after node i's Process.
    // What the hook records executes in that place of the frame.  Without a hook Process() records what it always did.
    static constexpr int CaptureSlotFrameStart = 0, CaptureSlotBeforeNodes = 1, CaptureSlotFirstNode = 2;
    using FrameCaptureHook = std::function<void(RHI::RHICommandListPtr cmdList, int slot)>;
    void CaptureNextFrame(FrameCaptureHook hook) { m_captureHook = std::move(hook); }
    bool IsCaptureArmed() const { return (bool)m_captureHook; }
    void Clear();

private:
    std::vector<FrameGraphNodePtr> m_graph;
    std::map<std::string, RHI::RHITexturePtr> m_renderTargets;
    std::map<std::string, RHI::RHITexturePtr> m_samplers;
    std::map<std::string, float> m_values;
    std::set<std::string> m_enabledNodes;
    RHI::ivec2 m_viewport;
    // RHIFrameGraph.h:72 `RHI::UboFrameData m_prevFrameData{}`: all zeros on a graph's first frame, afterwards what the last Process() uploaded as `frameData`
    // (RHIFrameGraph.cpp:189).  The reference builds a new RHIFrameGraph per `.renderer` file; here Clear() zeroes it with the graph.
    RHI::UboFrameData m_prevFrameData {};
    FrameCaptureHook m_captureHook;
};

} // namespace Sailor::Framegraph
